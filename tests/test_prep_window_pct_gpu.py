"""The percentile window on the device (csrc/prep_quantile.hip): effq_prep_quantiles bit for bit against numpy's sort of
the masked values, effq_prep_mask_window bit for bit against numpy.where(mask, numpy.clip), and the prep and predict
missions with --prep_window pLO,pHI against the restatement of tests/prep_window_ref.py."""
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, calibrate as K, config as Cf, data as D, entrance, predict, prep, synth
from efficientq_amd.hip_ops import get_ops
from tests import prep_spline_ref as S
from tests import prep_window_ref as Q
from tests import test_prep_cpu as R
from tests.test_prep_antialias_gpu import Recorder, _lits_set

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24
MODS = D.MODALITIES["brats"]


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ws_bytes(ops):
    need = C.c_size_t()
    assert ops.lib.effq_prep_quantile_ws_bytes(C.byref(need)) == _lib.EFFQ_OK
    return int(need.value)


def workspace(ops):
    ws = ops._workspace("prep_quantile", ws_bytes(ops))
    ws.fill_(0xFF)                       # the call clears what it counts in
    return ws


def check(ops, x, qs, mask):
    """x (C, S): count and statistics of two calls, equal to each other and to the sorted masked values bit for bit."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    t = dev(x)
    workspace(ops)
    count, stats = ops.prep_quantiles(t, qs, mask)
    workspace(ops)
    again = ops.prep_quantiles(t, qs, mask)
    assert torch.equal(count, again[0]) and torch.equal(stats.view(torch.int32), again[1].view(torch.int32))
    assert torch.equal(t.view(torch.int32), dev(x).view(torch.int32))                  # x is not modified
    count, stats = count.cpu().numpy(), stats.cpu().numpy()
    assert count.dtype == np.int64 and stats.dtype == np.float32 and stats.shape == (x.shape[0], len(qs), 2)
    for c in range(x.shape[0]):
        n, want = Q.ref_stats(x[c], qs, mask)
        assert count[c] == n, (c, count[c], n)
        assert Q.same_bits(stats[c], want), (c, qs, stats[c], want)
    return count, stats


def bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


# ---- shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_", [1, 2, 3, 5, 4099])
@pytest.mark.parametrize("mask", ["nonzero", "all"])
def test_statistics_equal_the_sorted_values_at_small_and_odd_sizes(ops, S_, mask):
    g = np.random.default_rng(S_)
    for Cc in (1, 2, 3, 4):
        x = (300.0 * g.standard_normal((Cc, S_))).astype(np.float32)
        for c in range(Cc):                                  # a zero margin of another width per modality
            x[c, :min(S_, c * (1 + S_ // 7))] = 0.0
            x[c, S_ - min(S_, 2 * c):] = 0.0
        count, _ = check(ops, x, (0.0, 37.5, 50.0, 100.0), mask)
        if mask == "nonzero" and Cc > 1 and S_ > 5:
            assert len(set(count.tolist())) == Cc            # the counts differ
        check(ops, x, (99.5,), mask)                         # R = 1


def test_second_trip_of_the_grid_stride_loop_with_a_tail(ops):
    S_ = 9 * 345 * 345
    assert S_ > 2 ** 20 and S_ % 4 == 1 and S_ // 4 > 1024 * 256      # more groups than one trip of the capped grid
    g = np.random.default_rng(9)
    x = (700.0 * g.standard_normal((2, S_))).astype(np.float32)
    x[1, g.random(S_) < 0.3] = 0.0
    x[:, -1] = (-1e6, 1e6)                                   # the tail voxel is the least of one and the greatest of the other
    count, stats = check(ops, x, (0.0, 0.5, 99.5, 100.0), "nonzero")
    assert count[0] == S_ and count[1] < 0.75 * S_
    assert stats[0, 0, 0] == -1e6 and stats[1, 3, 1] == 1e6


# ---- ties -----------------------------------------------------------------------------------------------------------------
def test_targets_inside_a_long_run_of_equal_values_on_its_first_and_on_its_last(ops):
    g = np.random.default_rng(70)
    n, below, run = 10001, 1000, 7000
    x = np.concatenate([g.uniform(-2000.0, -1001.0, below), np.full(run, -1000.0),
                        g.uniform(-999.0, 500.0, n - below - run)]).astype(np.float32)
    g.shuffle(x)
    qs = (9.995, 10.0, 50.0, 79.995)
    assert [Q.ref_rank(n, q)[1] for q in qs] == [below - 1, below, 5000, below + run - 1]
    _, stats = check(ops, x[None], qs, "all")
    assert stats[0, 0, 0] < -1000.0 and stats[0, 0, 1] == -1000.0        # steps onto the run's first element
    assert tuple(stats[0, 1]) == (-1000.0, -1000.0) and tuple(stats[0, 2]) == (-1000.0, -1000.0)
    assert stats[0, 3, 0] == -1000.0 and stats[0, 3, 1] > -1000.0        # steps off its last
    check(ops, np.stack([x, np.where(x == -1000.0, 0.0, x)]), qs, "nonzero")


def test_every_voxel_equal(ops):
    for v in (3.25, -1000.0):
        _, stats = check(ops, np.full((2, 4099), v, np.float32), (0.0, 50.0, 100.0), "all")
        assert np.all(stats == np.float32(v))


# ---- digits ---------------------------------------------------------------------------------------------------------------
def test_values_that_differ_in_one_byte_only(ops):
    g = np.random.default_rng(8)
    qs = (0.0, 33.3, 50.0, 100.0)
    low = bits(0x43801200 | g.integers(0, 256, 1003).astype(np.uint32))
    high = bits((g.integers(0, 256, 1003).astype(np.uint32) << 24) | 0x00400000)
    assert np.all(np.isfinite(high)) and len(np.unique(high)) > 200 and (high < 0).any() and (high > 0).any()
    second = bits(0xC2000034 | (g.integers(0, 256, 1003).astype(np.uint32) << 16) & 0x007F0000)
    for x in (low, high, second):
        check(ops, x[None], qs, "all")
        check(ops, x[None], qs, "nonzero")


def test_negative_and_positive_values_denormals_and_both_zeros(ops):
    g = np.random.default_rng(12)
    mixed = (g.standard_normal(4099) * 10.0 ** g.integers(-30, 30, 4099)).astype(np.float32)
    check(ops, mixed[None], (0.0, 25.0, 50.0, 100.0), "all")
    den = bits(g.integers(1, 0x800000, 2050).astype(np.uint32) | (g.integers(0, 2, 2050).astype(np.uint32) << 31))
    assert np.all(np.abs(den) < np.finfo(np.float32).tiny) and np.all(den != 0)
    count, _ = check(ops, den[None], (0.0, 25.0, 50.0, 100.0), "nonzero")      # a denormal is not zero
    assert count[0] == 2050
    zeros = np.concatenate([-g.random(10) - 1.0, np.resize(np.array([-0.0, 0.0]), 21), g.random(10) + 1.0])
    g.shuffle(zeros)
    _, stats = check(ops, zeros.astype(np.float32)[None], (30.0, 50.0, 70.0), "all")
    assert np.all(stats[0, :2] == 0.0) and not np.signbit(stats[0, :2]).any()   # +0.0 for a zero of either sign
    _, stats = check(ops, np.full((1, 7), -0.0, np.float32), (0.0, 100.0), "all")
    assert np.all(stats == 0.0) and not np.signbit(stats).any()


def test_infinities_sort_at_the_ends_and_nans_after_them(ops):
    g = np.random.default_rng(13)
    x = (100.0 * g.standard_normal(1001)).astype(np.float32)
    x[[3, 500]] = -np.inf
    x[[4, 1000]] = np.inf
    _, stats = check(ops, x[None], (0.0, 0.15, 50.0, 100.0), "all")
    assert tuple(stats[0, 0]) == (-np.inf, -np.inf) and stats[0, 1, 0] == -np.inf and np.isfinite(stats[0, 1, 1])
    assert tuple(stats[0, 3]) == (np.inf, np.inf)
    x[[7, 8, 900]] = bits([0x7FC00000, 0xFFC00000, 0x7F800001])           # quiet, negative and signalling NaNs: all last
    for mask in ("all", "nonzero"):
        _, stats = check(ops, x[None], (50.0, 99.75, 100.0), mask)
        assert np.all(np.isfinite(stats[0, 0])) and np.all(np.isnan(stats[0, 2]))
        assert stats[0, 1, 0] == np.inf and np.isnan(stats[0, 1, 1])       # +Inf, then the first NaN


# ---- ranks ----------------------------------------------------------------------------------------------------------------
def test_ranks_at_the_ends_integral_and_one_before_the_last(ops):
    g = np.random.default_rng(14)
    n = 4099
    x = (50.0 * g.standard_normal(n)).astype(np.float32)
    q_last = 100.0 * (n - 1.5) / (n - 1)
    assert Q.ref_rank(n, 50.0) == (2049.0, 2049) and Q.ref_rank(n, q_last)[1] == n - 2
    assert Q.ref_rank(n, 0.0)[1] == 0 and Q.ref_rank(n, 100.0)[1] == n - 1
    s = np.sort(x)
    _, stats = check(ops, x[None], (0.0, 50.0, q_last, 100.0), "all")
    assert tuple(stats[0, 0]) == (s[0], s[1]) and tuple(stats[0, 1]) == (s[2049], s[2050])
    assert tuple(stats[0, 2]) == (s[n - 2], s[n - 1]) and tuple(stats[0, 3]) == (s[n - 1], s[n - 1])
    for q in (0.0, 50.0, q_last, 100.0):                     # R = 1
        check(ops, x[None], (q,), "all")
    check(ops, np.array([[2.0, -1.0]], np.float32), (0.0, 50.0, 100.0), "all")        # n = 2


def test_an_empty_mask_gives_count_zero_and_nan_and_the_call_returns(ops):
    x = np.zeros((3, 4099), np.float32)
    x[1] = np.arange(4099)
    count, stats = check(ops, x, (1.0, 99.0), "nonzero")
    assert count.tolist() == [0, 4098, 0] and np.all(np.isnan(stats[[0, 2]])) and np.all(np.isfinite(stats[1]))


# ---- the masked window -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 4 * 256 * 3 + 5])
@pytest.mark.parametrize("mask", ["nonzero", "all"])
def test_window_mask_equals_numpy_where_of_clip(ops, n, mask):
    g = np.random.default_rng(n)
    x = (300.0 * g.standard_normal(n)).astype(np.float32)
    x[::5] = np.resize(np.array([-200.0, 250.0, np.inf, -np.inf, 250.00002, 0.0, -0.0, np.nan], np.float32), len(x[::5]))
    x[-1] = 1e4                                             # the tail is clipped too
    want = Q.ref_window_mask(x, -200.0, 250.0, mask)
    t = dev(x)
    assert ops.prep_window_mask(t, -200.0, 250.0, mask) is t
    assert Q.same_bits(t.cpu().numpy(), want)
    off = dev(np.concatenate([np.zeros(1, np.float32), x]))[1:]           # 4-B aligned only
    ops.prep_window_mask(off, -200.0, 250.0, mask)
    assert Q.same_bits(off.cpu().numpy(), want)
    # a window above zero: under `nonzero` the zeros stay zeros, under `all` they go up to the bound
    want = Q.ref_window_mask(x, 10.0, 250.0, mask)
    got = ops.prep_window_mask(dev(x), 10.0, 250.0, mask).cpu().numpy()
    assert Q.same_bits(got, want) and np.array_equal(got == 0, (x == 0) if mask == "nonzero" else np.zeros(n, bool))
    if mask == "all":
        assert Q.same_bits(got, ops.prep_window(dev(x), 10.0, 250.0).cpu().numpy())


# ---- bad arguments ----------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(ops):
    Cc, S_ = 2, 37
    x = dev(np.arange(1, Cc * S_ + 1, dtype=np.float32).reshape(Cc, S_))
    count = torch.full((Cc,), -7, dtype=torch.int64, device=DEV)
    stat = torch.full((Cc, 2, 2), 7.0, device=DEV)
    need = ws_bytes(ops)
    assert ops.lib.effq_prep_quantile_ws_bytes(None) == 1
    ws = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 8 == 0 and need > 0
    nan = float("nan")
    good = dict(x=x.data_ptr(), C=Cc, S=S_, mode=0, q=(1.0, 99.0), R=2, count=count.data_ptr(), stat=stat.data_ptr(),
                ws=ws.data_ptr(), bytes=need)

    def call(**over):
        a = dict(good, **over)
        q = (C.c_double * len(a["q"]))(*a["q"]) if a["q"] is not None else None
        return ops.lib.effq_prep_quantiles(a["x"], a["C"], a["S"], a["mode"], q, a["R"], a["count"], a["stat"], a["ws"],
                                           a["bytes"], ops.stream)
    bad = [dict(R=0), dict(R=-1), dict(R=5, q=(1.0, 2.0, 3.0, 4.0, 5.0)),
           dict(q=(-0.5, 99.0)), dict(q=(1.0, 100.5)), dict(q=(nan, 99.0)), dict(q=(1.0, nan)), dict(q=None),
           dict(x=None), dict(count=None), dict(stat=None), dict(ws=None),
           dict(bytes=need - 1), dict(bytes=0), dict(ws=ws.data_ptr() + 4),             # short, misaligned
           dict(x=x.data_ptr() + 2), dict(count=count.data_ptr() + 4), dict(stat=stat.data_ptr() + 2),
           dict(C=0), dict(C=-1), dict(C=5), dict(S=0), dict(S=-3), dict(S=2 ** 31), dict(C=2, S=2 ** 30),
           dict(mode=2), dict(mode=-1)]
    for over in bad:
        assert call(**over) == 1, over                                         # EFFQ_ERR_ARG
        assert b"argument check failed" in ops.lib.effq_last_error()
    y = torch.full((40,), 7.0, device=DEV)
    for a in ((None, 40, 0.0, 1.0, 0), (y.data_ptr(), 0, 0.0, 1.0, 0), (y.data_ptr(), 40, 2.0, 1.0, 0),
              (y.data_ptr(), 40, nan, 1.0, 0), (y.data_ptr(), 40, 0.0, nan, 0), (y.data_ptr(), 40, 0.0, 1.0, 2),
              (y.data_ptr() + 2, 39, 0.0, 1.0, 0)):
        assert ops.lib.effq_prep_mask_window(*a, ops.stream) == 1, a
        assert b"argument check failed" in ops.lib.effq_last_error()
    torch.cuda.synchronize()
    assert bool((count == -7).all()) and bool((stat == 7.0).all()) and bool((ws == 0x5A).all()) and bool((y == 7.0).all())
    assert call() == _lib.EFFQ_OK and call(q=(0.0, 100.0)) == _lib.EFFQ_OK    # what is legal: the ends of the range
    torch.cuda.synchronize()
    assert count.tolist() == [S_, S_] and stat[1].tolist() == [[S_ + 1.0, S_ + 2.0], [2.0 * S_, 2.0 * S_]]
    assert bool((ws[need:] == 0x5A).all())
    # the wrappers check as their neighbours do
    for bad_x, qs, mask in ((x.to(torch.float64), (1.0,), "nonzero"), (x[0], (1.0,), "nonzero"), (x, (), "nonzero"),
                            (x, (1.0, 2.0, 3.0, 4.0, 5.0), "nonzero"), (x, (101.0,), "nonzero"), (x, (nan,), "all"),
                            (x, (1.0,), "body"), (torch.zeros(5, 8, device=DEV), (1.0,), "all"), (x.cpu(), (1.0,), "all"),
                            (x.t(), (1.0,), "all")):
        with pytest.raises(_lib.EffqError):
            ops.prep_quantiles(bad_x, qs, mask)
    for lo, hi, mask in ((2.0, 1.0, "all"), (nan, 1.0, "all"), (0.0, 1.0, "body")):
        with pytest.raises(_lib.EffqError):
            ops.prep_window_mask(y, lo, hi, mask)
    with pytest.raises(_lib.EffqError):
        ops.prep_window_mask(y.to(torch.float64), 0.0, 1.0, "all")


# ---- the bounds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["nonzero", "all"])
def test_bounds_from_the_device_statistics_are_the_rule_and_numpys_percentile(ops, mask):
    g = np.random.default_rng(21)
    x = (g.gamma(2.0, 400.0, (4, 20011)) * (1.0 + np.arange(4))[:, None]).astype(np.float32)
    x[0] -= 900.0                                          # negative values too
    x[:, g.random(20011) < 0.4] = 0.0
    qs = (0.5, 1.0, 99.0, 99.5)
    count, stats = ops.prep_quantiles(dev(x), qs, mask)
    count, stats = count.cpu().tolist(), stats.cpu().numpy()
    for c in range(4):
        inside = x[c][Q.ref_mask(x[c], mask)].astype(np.float64)
        bound = Q.percentile_bound(x[c], mask)
        assert bound == U24 * np.abs(inside).max() + 2.0 ** -50 * len(inside) * (inside.max() - inside.min())
        for r, q in enumerate(qs):
            v = prep.percentile_value(count[c], q, stats[c, r, 0], stats[c, r, 1])
            assert np.float32(v).view(np.uint32) == Q.ref_percentile(x[c], q, mask).view(np.uint32)
            diff = abs(v - np.percentile(inside, q))
            print(f"{mask} c={c} p{q}: bound {v!r}, |bound - numpy.percentile| = {diff:.3e}, allowed {bound:.3e}")
            assert diff <= bound


# ---- end to end -----------------------------------------------------------------------------------------------------------
FACTORS, GRID, SPACING = (0.6, 1.4, 1.0), (33, 17, 28), "0.6,1.4,1"


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_prep_mission_windows_every_modality_by_its_own_percentiles_on_the_device(ops, tmp_path, capsys, interp):
    root = str(tmp_path)
    rows, truth = R.write_subjects(root, ["a", "b"], [5, 6], affine=np.eye(4))
    lst = R.write_list(tmp_path / "cases.csv", rows)
    kw = ["--task", "brats", "--src_list", lst, "--prep_spacing", SPACING, "--prep_min_size", "4,4,4", "--prep_interp",
          interp]
    plain, out = os.path.join(root, "plain"), os.path.join(root, "on")
    entrance.main(["prep", "--data_dir", plain] + kw)
    capsys.readouterr()
    entrance.main(["prep", "--data_dir", out, "--prep_window", "p1,p99"] + kw)
    said = capsys.readouterr().out
    table = list(csv.reader(open(os.path.join(out, prep.PREP_CSV))))
    assert table[0] == prep.prep_csv_header(MODS) + (["interp"] if interp == "cubic" else []) + prep.window_columns(MODS)
    before = {r["subject"]: r for r in csv.DictReader(open(os.path.join(plain, prep.PREP_CSV)))}
    for line in csv.DictReader(open(os.path.join(out, prep.PREP_CSV))):
        sn = line["subject"]
        x = truth[sn][0].astype(np.float32)
        assert (line["pmin"], line["pmax"]) == (before[sn]["pmin"], before[sn]["pmax"])      # the crop box is what it was
        box = tuple(slice(int(a), int(b)) for a, b in zip(line["pmin"].split(), line["pmax"].split()))
        for c, m in enumerate(MODS):
            lo, hi = (Q.ref_percentile(x[c], q, "nonzero") for q in (1.0, 99.0))
            assert line[f"{m}_win_lo"] == repr(float(lo)) and line[f"{m}_win_hi"] == repr(float(hi))
            assert f"{m} {float(lo):.7g} {float(hi):.7g}" in said
            inside = x[c][x[c] != 0]
            assert inside.min() < lo < hi < inside.max()
            clipped = Q.ref_window_mask(x[c], lo, hi, "nonzero")[None]
            if interp == "cubic":       # the masked window once more after the spline, with the same bounds
                res = S.ref_resample_cubic(clipped.astype(np.float64), FACTORS, GRID, zero_keep=True)
                assert res[res != 0].max() > hi + 1.0                                        # the spline overshoots
                e = float(S.ref_tolerance(res, float(hi)).max())
                res = np.where(res != 0, np.clip(res, np.float64(lo), np.float64(hi)), res)
            else:
                res = R.ref_resample_linear(clipped, FACTORS, GRID)
                e = 8 * U24 * float(hi)                      # the resampling's bound (test_prep_gpu.py), max |x| = hi
            body = res != 0
            mean, std = res[body].mean(), res[body].std()
            want = np.where(body, (res - mean) / std, 0.0)[0][box]
            arr = np.load(os.path.join(out, m, f"{sn}.npy"))
            assert arr.shape == want.shape and arr.dtype == np.float32
            assert np.array_equal(arr == 0, want == 0) and np.all(arr.view(np.uint32)[arr == 0] == 0)
            assert line[f"{m}_count"] == before[sn][f"{m}_count"] == str(int(body.sum()))
            # mean and std of the device's volume move by at most e each, then one float32 rounding
            tol = (2.0 + np.abs(want)) * e / std + np.spacing(np.abs(want).astype(np.float32))
            err = np.abs(arr.astype(np.float64) - want)
            print(f"{interp} {sn} {m}: window {float(lo)!r} {float(hi)!r}, worst err / bound = {(err / tol).max():.3e}")
            assert np.all(err <= tol)
            assert not np.array_equal(arr, np.load(os.path.join(plain, m, f"{sn}.npy")))
        assert open(os.path.join(out, "seg", f"{sn}.npy"), "rb").read() == \
            open(os.path.join(plain, "seg", f"{sn}.npy"), "rb").read()


def test_predict_windows_as_prep_does_and_names_the_bounds(ops, tmp_path, capsys):
    root = str(tmp_path)
    lst, truth = _lits_set(root)
    out = os.path.join(root, "data")
    target = "1.25,1.75,2"
    entrance.main(["prep", "--task", "lits", "--src_list", lst, "--data_dir", out, "--prep_spacing", target,
                   "--prep_window", "p1,p99", "--prep_min_size", "16,16,16"])
    capsys.readouterr()
    table = {r["subject"]: r for r in csv.DictReader(open(os.path.join(out, prep.PREP_CSV)))}
    bounds = {}
    for sn, (ct, _) in truth.items():
        lo, hi = (float(Q.ref_percentile(ct.astype(np.float32), q, "all")) for q in (1.0, 99.0))
        assert (table[sn]["ct_win_lo"], table[sn]["ct_win_hi"]) == (repr(lo), repr(hi)) and hi < 3000.0
        bounds[sn] = f"{lo:.7g} {hi:.7g}"
    args = Cf.make_args(Cf.TINY_NET, 4, 4)
    QConv, _, kwQ = Cf.get_conv_class(args)
    model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
    synth.randomise_network(model, 0)
    model.eval()
    K.search_fold_and_remove_bn(model)
    model.to(DEV)
    K.set_fp(model)
    seg = os.path.join(root, "seg")
    for k, v in dict(task="lits", src_list=lst, out_dir=seg, patch_size="16,16,16", prep_spacing=target,
                     prep_window="p1,p99", merge_type=None).items():
        setattr(args, k, v)
    rec = Recorder(ops)
    rows = predict.run(args, ops=rec, model=model, window_batch=8)
    said = capsys.readouterr().out
    assert [r["subject"] for r in rows] == ["l1", "l2"] and len(rec.arrays) == 2
    for r, y in zip(rows, rec.arrays):
        sn = r["subject"]
        assert np.array_equal(y[0].view(np.uint32), np.load(os.path.join(out, "ct", f"{sn}.npy")).view(np.uint32))
        assert f"{sn}: 40 48 56, window ct {bounds[sn]} -> grid" in said
    table = list(csv.reader(open(os.path.join(seg, predict.PREDICT_CSV))))
    assert table[0] == predict.CSV_HEADER + ["window_bounds"]
    col = table[0].index("prep_window")
    assert [r[col] for r in table[1:]] == ["p1 p99"] * 2 and [r[-1] for r in table[1:]] == [bounds["l1"], bounds["l2"]]
    assert sorted(os.listdir(seg)) == ["l1.nii.gz", "l2.nii.gz", "predict.csv"]
