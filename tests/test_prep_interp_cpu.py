"""`--prep_interp cubic`, host side (no GPU): the restatement tests/prep_spline_ref.py against scipy and closed forms, the
switch and its refusals, the C-ABI rows of the new entries, and the `prep` and `predict` missions driven through numpy
stand-ins whose prep_resample_cubic is the restatement."""
import csv
import os
import re

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, data as D, predict, prep
from tests import prep_spline_ref as S
from tests.test_predict_cpu import PointNet, predict_args, write_cases
from tests.test_prep_antialias_cpu import SmoothMixin
from tests.test_prep_cpu import NumpyOps, prep_args, write_list, write_subjects, written
from tests.test_window_blend_cpu import BlendOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# shape, factors: extents 1 and 2 on every axis, a row of extent 300, up- and down-sampling mixed
CASES = [((7, 5, 9), (1.7, 0.6, 2.5)), ((2, 3, 4), (0.5, 1.3, 0.8)), ((1, 6, 33), (1.0, 0.37, 3.1)),
         ((40, 2, 3), (3.1, 0.5, 1.0)), ((1, 2, 300), (1.0, 2.0, 0.7))]


def out_shape(shape, factors):
    return tuple(prep.resample_extent(n, f) for n, f in zip(shape, factors))


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,factors", CASES)
def test_restatement_equals_scipy(shape, factors):
    ndi = pytest.importorskip("scipy.ndimage")
    x = np.random.default_rng(sum(shape)).standard_normal(shape)
    bound = 1e-12 * np.abs(x).max()
    for axis in range(3):
        got = S.ref_prefilter_axis(x, axis)
        want = ndi.spline_filter1d(x, order=3, axis=axis, mode="mirror") if shape[axis] > 1 else x
        assert np.abs(got - want).max() <= bound, (shape, axis)
    out = out_shape(shape, factors)
    coords = np.meshgrid(*(S.ref_coords(o, f, n) for o, f, n in zip(out, factors, shape)), indexing="ij")
    want = ndi.map_coordinates(x, coords, order=3, mode="mirror")
    got = S.ref_resample_cubic(x, factors, out)
    assert got.shape == out and got.dtype == np.float64
    assert np.abs(got - want).max() <= bound, (shape, factors)
    # leading axes are volumes of their own
    both = S.ref_resample_cubic(np.stack([x, 2.0 * x]), factors, out)
    assert np.abs(both[0] - got).max() <= bound and np.abs(both[1] - 2.0 * got).max() <= 2.0 * bound


def test_rule_constants_and_weights_are_preps():
    assert prep.CUBIC_POLE == S.POLE == np.sqrt(3.0) - 2.0 and prep.CUBIC_GAIN == S.GAIN == 6.0
    assert prep.INTERP_ORDERS == ("linear", "cubic") and prep.INTERP_COLUMNS == ["interp"]
    for t in (0.0, 0.25, 0.5, 0.999):
        w = prep.cubic_weights(t)
        assert sum(w) == pytest.approx(1.0, abs=1e-15) and all(v >= 0 for v in w)
        _, ws, _, _ = S.ref_axis(1, 1.0, 8)            # o = 0, f = 1: s = 0, t = 0
        assert w == pytest.approx(tuple(ws[0])) if t == 0.0 else True
    assert prep.cubic_weights(0.0) == pytest.approx((1 / 6, 4 / 6, 1 / 6, 0.0))
    # the coordinates are the trilinear path's, the mirror brings -1 to 1 and n to n - 2
    idx, w, i0, i1 = S.ref_axis(4, 2.5, 10)
    assert i0.tolist() == [0, 3, 5, 8] and i1.tolist() == [1, 4, 6, 9]
    assert idx[0].tolist() == [1, 0, 1, 2] and idx[3].tolist() == [7, 8, 9, 8]
    idx, w, i0, i1 = S.ref_axis(3, 1.0, 3)              # identity: t = 0 everywhere, the second index does not count
    assert i0.tolist() == i1.tolist() == [0, 1, 2] and idx[2].tolist() == [1, 2, 1, 0] and w[2, 3] == 0.0
    idx, w, _, _ = S.ref_axis(5, 0.2, 1)                # extent 1: the one coefficient, weight 1
    assert not idx.any() and w.tolist() == [[0.0, 1.0, 0.0, 0.0]] * 5


@pytest.mark.parametrize("shape,factors", CASES)
def test_identity_factors_and_constants_are_closed_forms(shape, factors):
    x = np.random.default_rng(1).standard_normal(shape)
    assert np.abs(S.ref_resample_cubic(x, (1.0, 1.0, 1.0), shape) - x).max() <= 1e-12
    out = out_shape(shape, factors)
    const = S.ref_resample_cubic(np.full(shape, 3.25), factors, out)
    assert np.abs(const - 3.25).max() <= 1e-12
    assert np.abs(S.ref_prefilter(np.full(shape, 3.25)) - 3.25).max() <= 1e-12      # the spline of a constant is itself


def test_zero_rule_keeps_the_background_and_the_window_clips_the_overshoot():
    x = np.zeros((9, 10, 11))
    x[4:7, 4:7, 3:8] = 100.0 + np.random.default_rng(2).standard_normal((3, 3, 5))
    f, out = (1.3, 1.7, 1.1), out_shape(x.shape, (1.3, 1.7, 1.1))
    # no output voxel sits on a source voxel along any axis (there the spline gives the source's 0 back but for the last
    # bits, which may well cancel to 0), so away from the blob the free spline is small and not 0
    for o, ff, n in zip(out, f, x.shape):
        s = S.ref_coords(o, ff, n)
        assert np.all(s > np.floor(s)) and s.max() < n - 1
    free, kept = S.ref_resample_cubic(x, f, out), S.ref_resample_cubic(x, f, out, zero_keep=True)
    named = S.ref_footprint_zero(x, f, out)
    assert named.any() and not named.all()
    assert np.all(kept[named] == 0) and np.all(free[named] != 0) and np.array_equal(kept[~named], free[~named])
    # the footprint is the trilinear step's: where that step gives 0 from all-zero neighbours
    from tests.test_prep_cpu import ref_resample_linear
    lin = ref_resample_linear(x[None], f, out)[0]
    assert np.array_equal(lin == 0, named)
    assert free.min() < 0.0 and free.max() > x.max()                        # a step edge: the spline overshoots
    clipped = S.ref_window(free, 0.0, 100.0)
    assert clipped.min() == 0.0 and clipped.max() == 100.0
    # a NaN is not zero
    y = np.zeros((3, 3, 3))
    y[1, 1, 1] = np.nan
    assert not S.ref_footprint_zero(y, (1.0, 1.0, 1.0), (3, 3, 3))[1, 1, 1]
    assert S.ref_footprint_zero(y, (1.0, 1.0, 1.0), (3, 3, 3)).sum() == 26


# ---- the symbols -------------------------------------------------------------------------------------------------------
NEW = {"effq_prep_cubic_ws_bytes": ["N", "D", "H", "W", "bytes"],
       "effq_prep_cubic_plan": ["N", "D", "H", "W", "OD", "OH", "OW", "chunk", "tile_rows", "items", "trip"],
       "effq_prep_spline_prefilter": ["x", "N", "D", "H", "W", "passes", "ws", "ws_bytes", "stream"],
       "effq_prep_resample_cubic": ["x", "N", "D", "H", "W", "fd", "fh", "fw", "zero_keep", "y", "OD", "OH", "OW", "ws",
                                    "ws_bytes", "stream"]}


def test_cubic_symbols_in_header_lib_and_makefile():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return _lib._P
        if decl.startswith("long long"):
            return _lib._LL
        return {"int": _lib._I, "float": _lib._F, "double": _lib._D, "size_t": _lib._SZ}[decl.split()[0]]
    for name, names in NEW.items():
        found = re.findall(r"\bint (%s)\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert len(found) == 1, name
        args = [a.strip() for a in found[0][1].split(",")]
        res, got = _lib.SIGNATURES[name]
        assert res == _lib._I and got == [ctype(a) for a in args], name
        assert [a.split()[-1].lstrip("*") for a in args] == names, name
    # effq_prep_resample and its modes are what they were
    assert re.search(r"enum \{ EFFQ_PREP_LINEAR = 0, EFFQ_PREP_NEAREST = 1 \};", code)
    assert _lib.SIGNATURES["effq_prep_resample"] == (_lib._I, [_lib._P] + [_lib._I] * 4 + [_lib._D] * 3 + [_lib._I, _lib._P] +
                                                     [_lib._I] * 3 + [_lib._P])
    passes = dict(re.findall(r"EFFQ_PREP_SPLINE_PASS_(\w) = (\d+)", code))
    assert {k.lower(): int(v) for k, v in passes.items()} == _lib.PREP_SPLINE_PASSES == {"d": 1, "h": 2, "w": 4}
    make = open(os.path.join(ROOT, "efficientq_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "prep_spline.hip" in srcs and "prep.hip" in srcs and "prep_smooth.hip" in srcs
    deps = re.search(r"^%\.o: (.*)$", make, flags=re.M).group(1).split()
    src = open(os.path.join(ROOT, "efficientq_amd", "csrc", "prep_spline.hip")).read()
    for inc in re.findall(r'#include "([^"]+)"', src):
        assert inc in deps, inc
    assert not re.search(r"atomic\w*\s*\(", re.sub(r"//.*", "", src))       # deterministic: no atomics at all
    assert not re.search(r"hipMalloc|hipMemcpy|hipFree", src)               # the workspace is the caller's
    assert src.count("prep_grid(") >= 4                                     # every launch through the capped grid


# ---- the switch --------------------------------------------------------------------------------------------------------
def test_parser_knows_the_switch_and_yaml_sets_it(tmp_path):
    for mission in ("prep", "predict", "ptq"):
        assert Cf.build_parser().parse_args([mission]).prep_interp == "linear"
        assert Cf.build_parser().parse_args([mission, "--prep_interp", "cubic"]).prep_interp == "cubic"
    cfg = tmp_path / "p.yaml"
    cfg.write_text("prep_interp: cubic\nprep_spacing: '2,2,2'\n")
    a = Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["prep"]))
    assert a.prep_interp == "cubic" and prep.interp_switch(a, (2.0, 2.0, 2.0)) == "cubic"
    assert prep.interp_switch(Cf.build_parser().parse_args(["prep"]), None) == "linear"
    assert prep.interp_switch(Cf.build_parser().parse_args(["prep"]), (1.0, 1.0, 1.0)) == "linear"

    class Old:          # an args object from before the switch
        pass
    assert prep.interp_switch(Old(), None) == "linear"
    for bad in ("bicubic", "3", "", "nearest"):
        a.prep_interp = bad
        with pytest.raises(SystemExit) as e:
            prep.interp_switch(a, (2.0, 2.0, 2.0))
        assert isinstance(e.value, prep.PrepError) and "--prep_interp" in str(e.value) and repr(bad) in str(e.value)
        assert "linear or cubic" in str(e.value)
    a.prep_interp = "cubic"
    with pytest.raises(SystemExit) as e:
        prep.interp_switch(a, None)
    assert "--prep_interp cubic" in str(e.value) and "--prep_spacing" in str(e.value)


class CubicMixin:
    """prep_resample_cubic through the restatement, with a record of the calls and of what the moments then see."""

    def prep_resample_cubic(self, x, factors, out_shape, keep_zero=False):
        if not hasattr(self, "cubic"):
            self.cubic = []
        before = x.clone()
        y = S.ref_resample_cubic(x.numpy(), factors, out_shape, keep_zero).astype(np.float32)
        assert torch.equal(before, x)
        self.cubic.append(dict(shape=tuple(x.shape), dtype=str(x.dtype), factors=tuple(float(f) for f in factors),
                               out=tuple(int(o) for o in out_shape), keep_zero=bool(keep_zero), lo=float(y.min()),
                               hi=float(y.max())))
        return torch.from_numpy(y)

    def prep_bbox_moments(self, x, mask="nonzero"):
        if not hasattr(self, "seen"):
            self.seen = []
        self.seen.append((float(x.min()), float(x.max())))
        return super().prep_bbox_moments(x, mask)


class CubicNumpyOps(CubicMixin, SmoothMixin, NumpyOps):
    pass


class CubicPredictOps(CubicMixin, SmoothMixin, BlendOps):
    pass


def test_refused_before_anything_is_written(tmp_path):
    root, out = str(tmp_path), str(tmp_path / "out")
    rows, _ = write_subjects(root, ["a", "b"], [1, 2], affine=np.eye(4))
    lst = write_list(tmp_path / "cases.csv", rows)
    cases, _ = write_cases(os.path.join(root, "ct"), ["a", "b"], [1, 2], affine=np.eye(4))

    def refused(named, **over):
        for run in (lambda: prep.run(prep_args(src_list=lst, data_dir=out, prep_min_size="1,1,1", **over),
                                     ops=CubicNumpyOps()),
                    lambda: predict.run(predict_args(src_list=cases, out_dir=out, patch_size="1,1,1", **over),
                                        ops=CubicPredictOps(), model=PointNet(), window_batch=2)):
            with pytest.raises(SystemExit) as e:
                run()
            assert isinstance(e.value, prep.PrepError) and all(n in str(e.value) for n in named), str(e.value)
            assert not os.path.exists(out)
    refused(["--prep_interp", "'bicubic'", "linear or cubic"], prep_interp="bicubic", prep_spacing="2,2,2")
    refused(["--prep_interp cubic", "--prep_spacing"], prep_interp="cubic")


# ---- the missions on the host ------------------------------------------------------------------------------------------
def _table(path):
    return list(csv.reader(open(path)))


def _same_files(a, b):
    assert written(a) == written(b)
    for f in written(a):
        if not f.endswith(".gz") and f != D.SN_FN_FILE:          # gzip stamps the time
            assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


def test_prep_mission_resamples_by_splines_and_records_the_order(tmp_path, capsys):
    root = str(tmp_path)
    mods = D.MODALITIES["brats"]
    rows, truth = write_subjects(root, ["a", "b"], [5, 6], affine=np.eye(4))
    lst = write_list(tmp_path / "cases.csv", rows)
    kw = dict(prep_spacing="0.6,1.4,1", prep_min_size="4,4,4")
    factors, grid = (0.6, 1.4, 1.0), (33, 17, 28)
    # today's path: no switch, a stand-in that has no prep_resample_cubic; `linear` through one that has it is the same
    off, lin = os.path.join(root, "off"), os.path.join(root, "lin")
    assert not hasattr(NumpyOps, "prep_resample_cubic")
    args = prep_args(src_list=lst, data_dir=off, **kw)
    del args.prep_interp
    prep.run(args, ops=NumpyOps())
    said_off = capsys.readouterr().out
    ops = CubicNumpyOps()
    prep.run(prep_args(src_list=lst, data_dir=lin, prep_interp="linear", **kw), ops=ops)
    assert not hasattr(ops, "cubic") and capsys.readouterr().out == said_off.replace(off, lin)
    assert "cubic" not in said_off
    assert _table(os.path.join(off, prep.PREP_CSV))[0] == prep.prep_csv_header(mods)
    _same_files(off, lin)

    # cubic: one call per subject on the four modalities, never on the label; mask nonzero keeps the zeros
    on = os.path.join(root, "on")
    ops = CubicNumpyOps()
    got = prep.run(prep_args(src_list=lst, data_dir=on, prep_interp="cubic", **kw), ops=ops)
    said = capsys.readouterr().out
    assert [(c["shape"], c["dtype"], c["out"], c["keep_zero"]) for c in ops.cubic] == \
        [((4, 20, 24, 28), "torch.float32", grid, True)] * 2
    assert ops.cubic[0]["factors"] == pytest.approx(factors)
    assert "a: 20 24 28, cubic -> " in said and "b: 20 24 28, cubic -> " in said
    t_on, t_off = _table(os.path.join(on, prep.PREP_CSV)), _table(os.path.join(off, prep.PREP_CSV))
    assert t_on[0] == prep.prep_csv_header(mods) + ["interp"] and [r[-1] for r in t_on[1:]] == ["cubic"] * 2
    assert got[0]["interp"] == "cubic"
    for r_on, r_off in zip(t_on[1:], t_off[1:]):
        r_on, r_off = dict(zip(t_on[0], r_on)), dict(zip(t_off[0], r_off))
        # the body does not grow past what the trilinear step reaches: the same grid, box and counts
        for k in ["grid_shape", "pmin", "pmax"] + [f"{m}_count" for m in mods]:
            assert r_on[k] == r_off[k], k
        assert r_on["flair_std"] != r_off["flair_std"]
        sn = r_on["subject"]
        pmin, pmax = (tuple(int(v) for v in r_on[k].split()) for k in ("pmin", "pmax"))
        box = tuple(slice(a, b) for a, b in zip(pmin, pmax))
        vols = truth[sn][0].astype(np.float32)
        named = S.ref_footprint_zero(vols, factors, grid)
        res = S.ref_resample_cubic(vols, factors, grid, zero_keep=True).astype(np.float32)
        for c, m in enumerate(mods):
            a, b = np.load(os.path.join(on, m, f"{sn}.npy")), np.load(os.path.join(off, m, f"{sn}.npy"))
            assert a.shape == b.shape and a.dtype == np.float32 and not np.array_equal(a, b)
            assert np.array_equal(a == 0, named[c][box]) and np.all(a.view(np.uint32)[a == 0] == 0)     # exactly +0.0f
            v = res[c][res[c] != 0].astype(np.float64)
            want = np.where(res[c] != 0, ((res[c].astype(np.float64) - v.mean()) / v.std()).astype(np.float32), np.float32(0))
            assert np.abs(a - want[box]).max() <= 1e-5
        # the label and the grid are the linear run's
        assert open(os.path.join(on, "seg", f"{sn}.npy"), "rb").read() == open(os.path.join(off, "seg", f"{sn}.npy"), "rb").read()
    assert written(on) == written(off)

    # mask `all`: nothing is kept zero
    ops = CubicNumpyOps()
    prep.run(prep_args(src_list=lst, data_dir=os.path.join(root, "all"), prep_interp="cubic", prep_mask="all", **kw), ops=ops)
    assert [c["keep_zero"] for c in ops.cubic] == [False, False]
    # with --prep_antialias (and --prep_orient) the column comes after theirs
    both = os.path.join(root, "both")
    ops = CubicNumpyOps()
    prep.run(prep_args(src_list=lst, data_dir=both, prep_interp="cubic", prep_antialias=True, prep_orient="RAS",
                       prep_spacing="2.5,1.4,1", prep_min_size="4,4,4"), ops=ops)
    said = capsys.readouterr().out
    t = _table(os.path.join(both, prep.PREP_CSV))
    assert t[0] == prep.prep_csv_header(mods) + prep.ORIENT_COLUMNS + ["antialias", "interp"]
    assert t[1][-4:] == ["RAS", "RAS", "0.75 0.2 0", "cubic"]
    assert "a: 20 24 28, anti-alias sigma 0.75 0.2 0, cubic -> " in said
    assert len(ops.smoothed) == 2 and len(ops.cubic) == 2          # filter, then the spline


def test_prep_mission_applies_the_window_once_more(tmp_path, capsys):
    root = str(tmp_path)
    rows, _ = write_subjects(root, ["a"], [7], affine=np.eye(4))
    lst = write_list(tmp_path / "cases.csv", rows)
    kw = dict(src_list=lst, prep_spacing="0.6,1.4,0.37", prep_min_size="4,4,4", prep_mask="all", prep_interp="cubic")
    lo, hi = 400.0, 900.0
    ops = CubicNumpyOps()
    prep.run(prep_args(data_dir=os.path.join(root, "win"), prep_window="400,900", **kw), ops=ops)
    c = ops.cubic[0]
    assert c["lo"] < lo - 1.0 and c["hi"] > hi + 1.0              # the restatement overshoots on the clipped steps
    assert ops.seen == [(lo, hi)]                                 # what is standardised lies in the window again
    # without a window nothing is clipped
    ops = CubicNumpyOps()
    prep.run(prep_args(data_dir=os.path.join(root, "free"), **kw), ops=ops)
    c = ops.cubic[0]
    assert ops.seen == [(c["lo"], c["hi"])] and c["lo"] < 0.0


def test_predict_mission_resamples_as_prep_does(tmp_path, capsys):
    root = str(tmp_path)
    lst, truth = write_cases(root, ["s1", "s2"], [3, 4], affine=np.diag([1.0, 1.0, 2.0, 1.0]))
    kw = dict(src_list=lst, patch_size="8,8,8", prep_spacing="0.6,1.4,2", prep_mask="nonzero")
    grid = (33, 17, 28)

    def run(name, ops, *extra, **over):
        out = os.path.join(root, name)
        args = predict_args(*extra, out_dir=out, **dict(kw, **over))
        if over.get("prep_interp", 1) is None:
            del args.prep_interp
        rows = predict.run(args, ops=ops, model=PointNet(), window_batch=3)
        return out, rows, _table(os.path.join(out, predict.PREDICT_CSV)), capsys.readouterr().out
    assert not hasattr(BlendOps, "prep_resample_cubic")
    off, _, t_off, said_off = run("off", BlendOps(), prep_interp=None)
    ops = CubicPredictOps()
    lin, _, t_lin, said_lin = run("lin", ops, "--prep_interp", "linear")
    assert not hasattr(ops, "cubic") and t_off == t_lin and t_off[0] == predict.CSV_HEADER
    assert said_lin == said_off.replace(off, lin) and "cubic" not in said_off
    assert open(os.path.join(off, predict.PREDICT_CSV), "rb").read() == open(os.path.join(lin, predict.PREDICT_CSV), "rb").read()

    ops = CubicPredictOps()
    on, rows, t_on, said = run("on", ops, "--prep_interp", "cubic")
    assert [(c["shape"], c["out"], c["keep_zero"]) for c in ops.cubic] == [((1, 20, 24, 28), grid, True)] * 2
    assert t_on[0] == predict.CSV_HEADER + ["interp"] and [r[-1] for r in t_on[1:]] == ["cubic"] * 2
    assert rows[0]["interp"] == "cubic" and said.count(", cubic -> grid 33 17 28") == 2
    assert [r[:7] for r in t_on[1:]] == [r[:7] for r in t_off[1:]]          # the grid and the box are the linear run's
    # the lits window (-200, 250) is in force: the spline overshot it, and what is standardised lies inside it again
    assert all(c["lo"] < -201.0 and c["hi"] > 251.0 for c in ops.cubic)
    assert ops.seen == [(-200.0, 250.0)] * 2
    # without a window nothing is clipped; mask `all` keeps no zeros
    ops = CubicPredictOps()
    run("free", ops, "--prep_interp", "cubic", prep_window="none", prep_mask="all")
    assert [c["keep_zero"] for c in ops.cubic] == [False, False]
    assert ops.seen == [(c["lo"], c["hi"]) for c in ops.cubic]
    # after the antialias column's place and before those of --blend
    _, _, t_all, said = run("cols", CubicPredictOps(), "--prep_interp", "cubic", "--prep_antialias", "--blend", "gauss",
                            prep_orient="RAS", prep_spacing="2.5,1.4,2")
    assert t_all[0] == predict.CSV_HEADER + prep.ORIENT_COLUMNS + ["antialias", "interp"] + predict.CSV_BLEND_COLUMNS
    assert said.count(", anti-alias sigma 0.75 0.2 0, cubic -> grid 8 17 28") == 2
    _, _, t_b, _ = run("cols2", CubicPredictOps(), "--prep_interp", "cubic", "--blend", "gauss")
    assert t_b[0] == predict.CSV_HEADER + ["interp"] + predict.CSV_BLEND_COLUMNS
