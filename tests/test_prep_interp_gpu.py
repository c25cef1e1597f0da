"""effq_prep_resample_cubic (csrc/prep_spline.hip) against the fp64 restatement tests/prep_spline_ref.py, and
`--prep_interp cubic` end to end through the `prep` and `predict` missions on the device.

The bound is derived, not measured (prep_spline_ref.ref_tolerance): for `got` (float32 from the device) and `ref` (the
fp64 restatement)  |got - ref| <= 2^-24 |ref| + 2^-149 + 1e-11 max |x|: the one rounding to float32, plus an fp64
allowance for the order of the sums.  Every check prints its worst |got - ref| / bound before it asserts.  The shapes
that aim at the W pass's chunks and tiles and at the second trip of a capped grid come from effq_prep_cubic_plan."""
import csv
import gzip
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, calibrate as K, config as Cf, entrance, predict, prep, synth
from efficientq_amd.hip_ops import get_ops
from tests import prep_spline_ref as S
from tests import test_prep_cpu as R
from tests.test_prep_antialias_gpu import Recorder, _lits_set

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


@pytest.fixture(scope="module")
def plan0(ops):
    return ops.prep_cubic_plan((1, 2, 2, 2), (2, 2, 2))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def out_shape(shape, factors):
    return tuple(prep.resample_extent(n, f) for n, f in zip(shape[-3:], factors))


def volume(shape, seed=0, zeros=False):
    """CT-like values after the window; with `zeros` the first half of the longest axis is exactly 0."""
    g = np.random.default_rng(seed)
    x = np.clip(40.0 + 120.0 * g.standard_normal(shape), -200.0, 250.0).astype(np.float32)
    x[x == 0] = 1.0
    if zeros:
        a = 1 + int(np.argmax(shape[1:]))
        cut = [slice(None)] * 4
        cut[a] = slice(0, (shape[a] + 1) // 2)
        x[tuple(cut)] = 0.0
    return x


def check(ops, x, factors, keep_zero=False, out=None):
    out = out_shape(x.shape, factors) if out is None else out
    xd = dev(x)
    got = ops.prep_resample_cubic(xd, factors, out, keep_zero)
    again = ops.prep_resample_cubic(xd, factors, out, keep_zero)
    assert got.dtype == torch.float32 and tuple(got.shape) == (x.shape[0],) + tuple(out) and got.is_contiguous()
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))              # equal inputs, equal bits
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))      # x is not modified
    got = got.cpu().numpy()
    ref = S.ref_resample_cubic(x.astype(np.float64), factors, out, keep_zero)
    tol = S.ref_tolerance(ref, np.abs(x).max())
    ratio = float((np.abs(got.astype(np.float64) - ref) / tol).max())
    print(f"cubic {x.shape} f {factors} -> {out} keep_zero {keep_zero}: worst |got - ref| / bound = {ratio:.3e}")
    assert ratio <= 1.0
    if keep_zero:
        named = S.ref_footprint_zero(x, factors, out)
        assert np.all(got.view(np.uint32)[named] == 0)                              # exactly +0.0f
    return got


def check_all(ops, shape, factors, out=None, ns=(1, 3)):
    for n in ns:
        check(ops, volume((n,) + tuple(shape), seed=sum(shape) + n), factors, False, out)
        check(ops, volume((n,) + tuple(shape), seed=sum(shape) + n, zeros=True), factors, True, out)


SMALL = [((7, 5, 9), (1.7, 0.6, 2.5)),
         ((1, 6, 33), (0.6, 1.3, 0.8)), ((6, 1, 33), (1.3, 0.6, 0.8)), ((6, 33, 1), (0.8, 1.3, 0.6)),       # extent 1 ...
         ((2, 2, 2), (0.4, 0.6, 0.5)), ((2, 7, 5), (0.7, 1.0, 1.2)), ((7, 2, 5), (1.2, 0.7, 1.0)),           # ... and 2
         ((5, 7, 2), (1.0, 1.2, 0.7)),
         ((9, 8, 40), (0.37, 3.1, 0.37)), ((12, 9, 10), (3.1, 0.37, 3.1))]                                    # up and down


@pytest.mark.parametrize("shape,factors", SMALL)
def test_cubic_equals_the_restatement(ops, shape, factors):
    check_all(ops, shape, factors)


@pytest.mark.parametrize("which", ["chunk-1", "chunk", "chunk+1", "2chunk+3"])
def test_rows_at_the_chunk_boundaries_of_the_w_pass(ops, plan0, which):
    c = plan0["chunk"]
    W = {"chunk-1": c - 1, "chunk": c, "chunk+1": c + 1, "2chunk+3": 2 * c + 3}[which]
    assert c >= 3 and W >= 2
    check_all(ops, (2, 3, W), (1.0, 0.8, 0.9))


def test_tiles_of_the_w_pass_that_are_not_full(ops, plan0):
    rows = plan0["tile_rows"]
    # more than one tile, the last one partial, for N = 1 and N = 3; then fewer rows than one tile
    shape = (2, rows // 2 + 3, 5)
    for n in (1, 3):
        p = ops.prep_cubic_plan((n,) + shape, out_shape(shape, (1.0, 1.3, 0.8)))
        assert p["items"]["w"] == n * shape[0] * shape[1] > rows and p["items"]["w"] % rows != 0
    check_all(ops, shape, (1.0, 1.3, 0.8))
    shape = (1, rows // 4, 5)
    assert ops.prep_cubic_plan((3,) + shape, (1, 1, 1))["items"]["w"] < rows
    check_all(ops, shape, (1.0, 1.3, 0.8))


@pytest.mark.parametrize("OW", [1, 3, 4, 5])
def test_the_tail_of_the_16_byte_store(ops, OW):
    shape, f = (3, 4, 10), (0.75, 1.0, 10.0 / OW)
    assert out_shape(shape, f)[2] == OW
    check_all(ops, shape, f)


def _second_trip(ops, name, shape, factors):
    """N = 3 volumes of `shape`: the launch `name` has more work items than one trip of its capped grid covers."""
    out = out_shape(shape, factors)
    p = ops.prep_cubic_plan((3,) + shape, out)
    assert p["trip"][name] < p["items"][name] <= 2 * p["trip"][name], p
    check(ops, volume((3,) + shape, seed=11), factors, False)
    check(ops, volume((3,) + shape, seed=12, zeros=True), factors, True)


def _side(ops, name):
    """The least L with 3 * L * L lines (rows) above one trip of the launch `name`: three volumes, the filtered axis of
    extent 2 and the two others of extent L."""
    big = ops.prep_cubic_plan((3, 300, 300, 300), (300, 300, 300))      # the capped grid's trip
    trip = big["trip"][name]
    assert big["items"][name] > trip
    L = int(np.sqrt(trip / 3.0)) + 1
    assert 3 * L * L > trip
    return L


def test_second_trip_of_the_d_pass(ops):
    L = _side(ops, "d")
    _second_trip(ops, "d", (2, L, L), (1.0, 2.0, 2.0))


def test_second_trip_of_the_h_pass(ops):
    L = _side(ops, "h")
    _second_trip(ops, "h", (L, 2, L), (2.0, 1.0, 2.0))


def test_second_trip_of_the_w_pass(ops):
    L = _side(ops, "w")
    _second_trip(ops, "w", (L, L, 2), (2.0, 2.0, 1.0))


def test_second_trip_of_the_evaluation(ops):
    big = ops.prep_cubic_plan((3, 300, 300, 300), (300, 300, 300))
    trip = big["trip"]["eval"]
    # 3 * 6 * OH * (OW / 4) items with OH = OW = 4 L: 72 L^2 of them
    L = int(np.sqrt(trip / 72.0)) + 1
    _second_trip(ops, "eval", (3, L, L), (0.5, 0.25, 0.25))


def test_the_plan_query_counts_lines_rows_and_items(ops):
    p = ops.prep_cubic_plan((3, 5, 6, 7), (2, 9, 10))
    assert p["items"] == {"d": 3 * 6 * 7, "h": 3 * 5 * 7, "w": 3 * 5 * 6, "eval": 3 * 2 * 9 * 3}
    assert all(p["trip"][k] >= p["items"][k] for k in p["items"]) and p["chunk"] >= 3 and p["tile_rows"] >= 1
    p = ops.prep_cubic_plan((2, 5, 1, 1), (5, 1, 1))
    assert p["items"] == {"d": 2, "h": 0, "w": 0, "eval": 10} and p["trip"]["h"] == 0 == p["trip"]["w"]
    with pytest.raises(_lib.EffqError):
        ops.prep_cubic_plan((1, 0, 2, 2), (1, 1, 1))
    with pytest.raises(_lib.EffqError):
        ops.prep_cubic_plan((1, 2, 2, 40000), (1, 1, 1))


def test_the_prefilter_passes_give_the_coefficients(ops):
    for shape in ((2, 7, 5, 9), (1, 1, 6, 70), (1, 40, 2, 3)):
        x = volume(shape, seed=5)
        want = S.ref_prefilter(x.astype(np.float64))
        c = ops.prep_spline_prefilter(dev(x))
        assert c.dtype == torch.float64 and tuple(c.shape) == shape
        err = float(np.abs(c.cpu().numpy() - want).max())
        print(f"prefilter {shape}: max err {err:.3e}, bound {1e-11 * np.abs(x).max():.3e}")
        assert err <= 1e-11 * np.abs(x).max()
        # one pass at a time is the same arithmetic
        one = ops.prep_spline_prefilter(dev(x), "d")
        assert np.abs(one.cpu().numpy() - S.ref_prefilter_axis(x.astype(np.float64), -3)).max() <= 1e-11 * np.abs(x).max()
        ops.prep_spline_prefilter(dev(x), "h", out=one)
        ops.prep_spline_prefilter(dev(x), "w", out=one)
        assert torch.equal(one.view(torch.int64), c.view(torch.int64))
    with pytest.raises(_lib.EffqError):
        ops.prep_spline_prefilter(dev(volume((1, 2, 2, 2))), "hw")
    with pytest.raises(_lib.EffqError):
        ops.prep_spline_prefilter(dev(volume((1, 2, 2, 2))), "x")


# ---- closed forms --------------------------------------------------------------------------------------------------------
def test_identity_factors_give_the_input_back_and_a_constant_stays(ops):
    for shape in ((3, 7, 5, 9), (1, 2, 1, 70)):
        x = volume(shape, seed=3)
        got = check(ops, x, (1.0, 1.0, 1.0))
        tol = S.ref_tolerance(x.astype(np.float64), np.abs(x).max())
        assert np.all(np.abs(got.astype(np.float64) - x) <= tol)
        const = np.full(shape, 1234.5, np.float32)
        got = check(ops, const, (0.6, 1.7, 0.37))
        assert np.all(np.abs(got.astype(np.float64) - 1234.5) <= S.ref_tolerance(np.float64(1234.5), 1234.5))


# ---- the zero rule -------------------------------------------------------------------------------------------------------
def test_a_blob_inside_zeros_keeps_its_background_exactly_zero(ops):
    x = np.zeros((3, 9, 10, 11), np.float32)
    x[:, 4:7, 4:7, 3:8] = (100.0 + np.random.default_rng(2).standard_normal((3, 3, 3, 5))).astype(np.float32)
    f = (1.3, 1.7, 1.1)
    out = out_shape(x.shape, f)
    # no output voxel sits on a source voxel along any axis: there the free spline would give the source's 0 back but
    # for its last bits, which may cancel to 0; here it is small and not 0 wherever the rule names a voxel
    for o, ff, n in zip(out, f, x.shape[1:]):
        s = S.ref_coords(o, ff, n)
        assert np.all(s > np.floor(s)) and s.max() < n - 1
    named = S.ref_footprint_zero(x, f, out)
    ref = S.ref_resample_cubic(x.astype(np.float64), f, out)
    assert named.any() and not named.all() and np.abs(ref[named]).min() > 1e-30
    kept, free = check(ops, x, f, True), check(ops, x, f, False)
    assert np.all(kept.view(np.uint32)[named] == 0)                     # every voxel the footprint rule names: +0.0f
    assert np.all(kept[~named] != 0)
    assert np.all(free[named] != 0)                                     # without the rule the same voxels are not 0
    assert np.array_equal(kept.view(np.uint32)[~named], free.view(np.uint32)[~named])

    def box(a):
        idx = np.nonzero(a)
        return [(int(i.min()), int(i.max())) for i in idx]
    assert box(kept) == box(S.ref_resample_cubic(x.astype(np.float64), f, out, zero_keep=True))
    assert box(kept) != box(free)
    # a NaN is not zero, -0.0 is
    y = np.zeros((1, 3, 3, 3), np.float32)
    y[0, 1, 1, 1] = np.nan
    y[0, 0, 0, 0] = -0.0
    got = ops.prep_resample_cubic(dev(y), (1.0, 1.0, 1.0), (3, 3, 3), True).cpu().numpy()
    assert np.isnan(got[0, 1, 1, 1]) and (got.view(np.uint32) == 0).sum() == 26


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(ops):
    shape, f, out = (2, 4, 5, 6), (0.8, 1.0, 1.5), (5, 5, 4)
    n, no = int(np.prod(shape)), 2 * 5 * 5 * 4
    x = dev(volume(shape))
    y = torch.full((no + 8,), 7.0, device=DEV)
    ws = torch.full((n + 8,), 7.0, dtype=torch.float64, device=DEV)
    good = dict(x=x.data_ptr(), dims=shape, f=f, kz=0, y=y.data_ptr(), out=out, ws=ws.data_ptr(), nb=8 * n)

    def call(**over):
        a = dict(good, **over)
        return ops.lib.effq_prep_resample_cubic(a["x"], *a["dims"], *a["f"], a["kz"], a["y"], *a["out"], a["ws"], a["nb"],
                                                ops.stream)
    nan, inf = float("nan"), float("inf")
    bad = [dict(x=None), dict(y=None), dict(ws=None),
           dict(x=x.data_ptr() + 2), dict(y=y.data_ptr() + 1), dict(y=y.data_ptr() + 2),        # 4-B alignment of x and y
           dict(ws=ws.data_ptr() + 4), dict(ws=ws.data_ptr() + 1),                               # 8-B alignment of ws
           dict(nb=8 * n - 1), dict(nb=0), dict(nb=4 * n),
           dict(f=(0.0, 1.0, 1.5)), dict(f=(0.8, -1.0, 1.5)), dict(f=(0.8, 1.0, nan)), dict(f=(inf, 1.0, 1.5)),
           dict(f=(0.8, 1.0000001e6, 1.5)), dict(f=(nan, nan, nan)),
           dict(kz=2), dict(kz=-1),
           dict(dims=(0, 4, 5, 6)), dict(dims=(2, 0, 5, 6)), dict(dims=(2, 4, 5, 0)), dict(dims=(2, 4, 5, -6)),
           dict(dims=(1, 1, 1, 32768)), dict(dims=(1, 32768, 1, 1)), dict(dims=(3, 32767, 32767, 1)),
           dict(out=(0, 5, 4)), dict(out=(5, 5, -4)), dict(out=(5, 32768, 4)), dict(out=(32767, 32767, 2))]
    for over in bad:
        assert call(**over) == 1, over                                         # EFFQ_ERR_ARG
        assert b"argument check failed" in ops.lib.effq_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((ws == 7.0).all())                  # nothing was launched
    # what is legal: 4-B aligned x and y that are not 16-B aligned, a factor of 1e6, a workspace of exactly the size
    import ctypes as C
    need = C.c_size_t()
    assert ops.lib.effq_prep_cubic_ws_bytes(*shape, C.byref(need)) == _lib.EFFQ_OK and need.value == 8 * n
    assert ops.lib.effq_prep_cubic_ws_bytes(2, 4, 5, 40000, C.byref(need)) == 1
    xs = torch.zeros(n + 1, device=DEV)[1:]
    xs.copy_(x.reshape(-1))
    assert xs.data_ptr() % 16 == 4 and (y.data_ptr() + 4) % 16 == 4
    assert call(x=xs.data_ptr(), y=y.data_ptr() + 4) == _lib.EFFQ_OK
    torch.cuda.synchronize()
    want = ops.prep_resample_cubic(x, f, out)
    assert torch.equal(y[1:1 + no].view(torch.int32), want.reshape(-1).view(torch.int32))
    assert float(y[0]) == 7.0 and bool((y[1 + no:] == 7.0).all()) and bool((ws[n:] == 7.0).all())
    assert call(f=(1e6, 1.0, 1.5), out=(1, 5, 4)) == _lib.EFFQ_OK
    torch.cuda.synchronize()
    # the wrapper validates like prep_resample
    for badf, bado in (((0.0, 1.0, 1.0), out), ((1.0, 1.0), out), (f, (5, 5)), (f, (0, 5, 4)), ((nan, 1.0, 1.0), out)):
        with pytest.raises(_lib.EffqError):
            ops.prep_resample_cubic(x, badf, bado)
    with pytest.raises(_lib.EffqError):
        ops.prep_resample_cubic(x.to(torch.float64), f, out)


# ---- end to end ----------------------------------------------------------------------------------------------------------
SOURCE, SPACING, TARGET = (40, 48, 56), (0.5, 1.25, 2.0), "0.4,1.75,1.5"        # factors 0.8, 1.4, 0.75
WINDOW = (-200.0, 250.0)


class CubicRecorder(Recorder):
    """... and of what effq_prep_resample_cubic returned (before the window clips it) and of what the moments see."""

    def __init__(self, ops):
        super().__init__(ops)
        self.cubic, self.seen = [], []

    def prep_resample_cubic(self, *a, **kw):
        y = self._ops.prep_resample_cubic(*a, **kw)
        self.cubic.append(y.cpu().numpy())
        return y

    def prep_bbox_moments(self, x, *a, **kw):
        self.seen.append((float(x.min()), float(x.max())))
        return self._ops.prep_bbox_moments(x, *a, **kw)


def test_prep_and_predict_missions_interpolate_on_the_device(ops, tmp_path, capsys):
    root = str(tmp_path)
    lst, truth = _lits_set(root)
    factors = (0.8, 1.4, 0.75)
    grid = tuple(prep.resample_extent(n, f) for n, f in zip(SOURCE, factors))
    assert grid == (50, 34, 75)
    common = ["--task", "lits", "--src_list", lst, "--prep_spacing", TARGET, "--prep_window", "-200,250",
              "--prep_min_size", "16,16,16"]
    lin, out = os.path.join(root, "lin"), os.path.join(root, "data")
    entrance.main(["prep", "--data_dir", lin] + common)
    capsys.readouterr()
    args = Cf.build_parser().parse_args(["prep", "--data_dir", out, "--prep_interp", "cubic"] + common)
    rec = CubicRecorder(ops)
    prep.run(args, ops=rec)
    said = capsys.readouterr().out
    table = list(csv.DictReader(open(os.path.join(out, prep.PREP_CSV))))
    assert [r["subject"] for r in table] == ["l1", "l2"] and list(table[0])[-1] == "interp"
    arrays = {}
    for k, r in enumerate(table):
        sn = r["subject"]
        assert r["interp"] == "cubic" and r["grid_shape"] == "50 34 75"
        assert f"{sn}: 40 48 56, cubic -> 50 34 75" in said
        x = np.clip(truth[sn][0].astype(np.float32), np.float32(WINDOW[0]), np.float32(WINDOW[1]))[None]
        res = S.ref_resample_cubic(x.astype(np.float64), factors, grid)                     # fp64, mask `all`: no zero rule
        # before the standardisation: the device's resampled array against the restatement, within the kernel's bound
        tol = S.ref_tolerance(res, 250.0)
        ratio = float((np.abs(rec.cubic[k].astype(np.float64) - res) / tol).max())
        print(f"{sn}: resampled, worst |got - ref| / bound = {ratio:.3e}")
        assert ratio <= 1.0
        assert res.min() < WINDOW[0] - 1.0 and res.max() > WINDOW[1] + 1.0                   # the spline overshoots ...
        assert rec.seen[k] == WINDOW                                                        # ... and the window clips it
        # after it: the clip moves nothing apart, mean and std of the device's volume move by at most e each, then one
        # float32 rounding
        v = S.ref_window(res, *WINDOW)
        mean, std = v.mean(), v.std()
        want = (v - mean) / std
        arr = arrays[sn] = np.load(os.path.join(out, "ct", f"{sn}.npy"))
        assert arr.shape == grid and arr.dtype == np.float32
        e = float(tol.max())
        bound = (2.0 + np.abs(want[0])) * e / std + np.spacing(np.abs(want[0]).astype(np.float32))
        err = np.abs(arr.astype(np.float64) - want[0])
        print(f"{sn}: standardised, worst err / bound = {(err / bound).max():.3e}")
        assert np.all(err <= bound)
        assert not np.array_equal(arr, np.load(os.path.join(lin, "ct", f"{sn}.npy")))
        # the label and the grid image are the linear run's, byte for byte
        assert open(os.path.join(out, "seg", f"{sn}.npy"), "rb").read() == open(os.path.join(lin, "seg", f"{sn}.npy"), "rb").read()
        assert np.array_equal(np.load(os.path.join(out, "seg", f"{sn}.npy")),
                              R.ref_resample_nearest(truth[sn][1][None], factors, grid)[0])
        g_on, g_lin = (gzip.open(os.path.join(d, prep.GRID_DIR, f"{sn}.nii.gz")).read() for d in (out, lin))
        assert g_on == g_lin

    # predict with the same switches: the same working arrays, and the column in predict.csv
    args = Cf.make_args(Cf.TINY_NET, 4, 4)
    QConv, _, kwQ = Cf.get_conv_class(args)
    model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
    synth.randomise_network(model, 0)
    model.eval()
    K.search_fold_and_remove_bn(model)
    model.to(DEV)
    K.set_fp(model)
    seg = os.path.join(root, "seg")
    for k, v in dict(task="lits", src_list=lst, out_dir=seg, patch_size="16,16,16", prep_spacing=TARGET,
                     prep_interp="cubic", prep_window="-200,250", merge_type=None).items():
        setattr(args, k, v)
    rec = Recorder(ops)
    rows = predict.run(args, ops=rec, model=model, window_batch=8)
    said = capsys.readouterr().out
    assert [r["subject"] for r in rows] == ["l1", "l2"] and len(rec.arrays) == 2
    for r, y in zip(rows, rec.arrays):
        assert np.array_equal(y[0].view(np.uint32), arrays[r["subject"]].view(np.uint32))
        assert f"{r['subject']}: 40 48 56, cubic -> grid 50 34 75" in said
    table = list(csv.reader(open(os.path.join(seg, predict.PREDICT_CSV))))
    assert table[0] == predict.CSV_HEADER + ["interp"] and [r[-1] for r in table[1:]] == ["cubic"] * 2
    assert sorted(os.listdir(seg)) == ["l1.nii.gz", "l2.nii.gz", "predict.csv"]


def test_prep_mission_keeps_the_brats_background_exactly_zero_on_the_device(ops, tmp_path, capsys):
    root = str(tmp_path)
    rows, truth = R.write_subjects(root, ["a"], [5], affine=np.eye(4))
    lst = R.write_list(tmp_path / "cases.csv", rows)
    factors, grid = (0.6, 1.4, 1.0), (33, 17, 28)
    kw = ["--task", "brats", "--src_list", lst, "--prep_spacing", "0.6,1.4,1", "--prep_min_size", "4,4,4"]
    lin, out = os.path.join(root, "lin"), os.path.join(root, "on")
    entrance.main(["prep", "--data_dir", lin] + kw)
    entrance.main(["prep", "--data_dir", out, "--prep_interp", "cubic"] + kw)
    r_on, r_lin = (list(csv.DictReader(open(os.path.join(d, prep.PREP_CSV))))[0] for d in (out, lin))
    for k in ("grid_shape", "pmin", "pmax", "flair_count", "t2_count"):
        assert r_on[k] == r_lin[k], k                       # the body reaches no further than under the trilinear step
    pmin, pmax = (tuple(int(v) for v in r_on[k].split()) for k in ("pmin", "pmax"))
    box = tuple(slice(a, b) for a, b in zip(pmin, pmax))
    named = S.ref_footprint_zero(truth["a"][0].astype(np.float32), factors, grid)
    for c, m in enumerate(("flair", "t1", "t1ce", "t2")):
        a = np.load(os.path.join(out, m, "a.npy"))
        assert np.array_equal(a == 0, named[c][box]) and np.all(a.view(np.uint32)[a == 0] == 0)
    assert open(os.path.join(out, "seg", "a.npy"), "rb").read() == open(os.path.join(lin, "seg", "a.npy"), "rb").read()
    g_on, g_lin = (gzip.open(os.path.join(d, prep.GRID_DIR, "a.nii.gz")).read() for d in (out, lin))
    assert g_on == g_lin
