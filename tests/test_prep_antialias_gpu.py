"""effq_prep_smooth (csrc/prep_smooth.hip) against the fp64 restatement tests/prep_smooth_ref.py cast to float32, and
`--prep_antialias` end to end through the `prep` and `predict` missions on the device.

The bound is the arithmetic's, not a measured one (prep_smooth_ref.ref_bound): per filtered axis the device forms an
fp32 sum of 2 r + 1 products with float32 taps, (2 r + 3) 2^-24 max |x|, and the later passes, being averages, do not
amplify the earlier ones' error: the bounds of the filtered axes add."""
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, calibrate as K, config as Cf, entrance, predict, prep, synth
from efficientq_amd.hip_ops import get_ops
from tests import prep_smooth_ref as S
from tests import test_prep_cpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24
SIGMA = {0: 0.0, 1: 0.2, 3: 0.75, 7: 1.7, 12: 3.0, 32: 8.0}      # a sigma of every radius the cases use


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sigmas_of(radii):
    s = tuple(SIGMA[r] for r in radii)
    assert tuple(S.ref_radius(v) for v in s) == tuple(radii)
    return s


def volume(shape, seed=0):
    """CT-like values after the window: a smooth ramp plus noise within -200 ... 250."""
    g = np.random.default_rng(seed)
    return np.clip(40.0 + 120.0 * g.standard_normal(shape), -200.0, 250.0).astype(np.float32)


def check(ops, x, radii, keep_zero=False):
    s = sigmas_of(radii)
    got = ops.prep_smooth(dev(x), s, keep_zero)
    again = ops.prep_smooth(dev(x), s, keep_zero)
    assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))              # equal inputs, equal bits
    got = got.cpu().numpy()
    want = S.ref_smooth(x, s, keep_zero).astype(np.float32)
    bound = S.ref_bound(x, s)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"smooth {x.shape} radii {radii} keep_zero {keep_zero}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    return got


CASES = [(shape, radii)
         for W in (3, 5, 13, 70)
         for shape in ((1, 6, 7, W),)
         for radii in ((3, 0, 0), (0, 3, 1), (1, 1, 1), (0, 0, 3))]
CASES += [((1, 3, 4, 70), (0, 0, 32)), ((1, 3, 4, 5), (0, 0, 32)),                  # the widest window, also past both ends
          ((1, 3, 4, 70), (0, 0, 7)), ((1, 3, 4, 13), (0, 0, 7)),                    # the windows of 8 and of 16
          ((1, 3, 4, 70), (0, 0, 12)), ((1, 3, 4, 13), (0, 0, 12)),
          ((1, 2, 6, 7), (3, 0, 0)), ((1, 5, 2, 7), (0, 3, 0)), ((1, 5, 6, 2), (0, 0, 3)),   # both clamps in one stencil
          ((1, 2, 2, 2), (3, 3, 3)), ((1, 1, 1, 1), (1, 1, 1)),
          ((1, 40, 5, 9), (32, 0, 0)), ((1, 5, 40, 9), (0, 32, 0)),
          ((4, 6, 7, 13), (3, 1, 3)), ((4, 6, 7, 13), (1, 3, 0))]                    # N = 4: rows of other volumes stay out


@pytest.mark.parametrize("shape,radii", CASES)
def test_smooth_equals_the_restatement(ops, shape, radii):
    x = volume(shape, seed=sum(shape) + sum(radii))
    check(ops, x, radii)
    x[:, :, ::2, ::3] = 0.0
    check(ops, x, radii, keep_zero=True)


def test_second_trip_of_the_grid_stride_loop(ops):
    shape = (4, 64, 64, 80)
    assert shape[0] * shape[1] * shape[2] * (shape[3] // 4) > 1024 * 256          # more items than the capped grid's threads
    x = volume(shape, 3)
    got = check(ops, x, (1, 1, 1))
    assert not np.array_equal(got, x)


def test_base_pointers_aligned_to_four_bytes_only(ops):
    shape, radii = (2, 5, 6, 13), (3, 1, 3)
    n = int(np.prod(shape))
    x = volume(shape, 5)
    bufs = [torch.zeros(n + 1, device=DEV) for _ in range(3)]
    xs, ys, ts = (b[1:] for b in bufs)
    assert all(t.data_ptr() % 16 == 4 for t in (xs, ys, ts))
    xs.copy_(dev(x).reshape(-1))
    taps = [prep.antialias_taps(s) for s in sigmas_of(radii)]
    rc = ops.lib.effq_prep_smooth(xs.data_ptr(), *shape, taps[0].ctypes.data, radii[0], taps[1].ctypes.data, radii[1],
                                  taps[2].ctypes.data, radii[2], 0, ys.data_ptr(), ts.data_ptr(), ops.stream)
    assert rc == _lib.EFFQ_OK
    torch.cuda.synchronize()
    want = ops.prep_smooth(dev(x), sigmas_of(radii))
    assert torch.equal(ys.view(torch.int32), want.reshape(-1).view(torch.int32))
    assert all(float(b[0]) == 0.0 for b in bufs)                                   # nothing written in front of the base


def test_an_impulse_gives_the_outer_product_of_the_taps(ops):
    radii = (3, 1, 3)
    x = np.zeros((1, 9, 5, 13), np.float32)
    x[0, 4, 2, 6] = 1.0
    got = check(ops, x, radii)
    gd, gh, gw = (S.ref_taps(s) for s in sigmas_of(radii))
    want = np.zeros(x.shape)
    want[0, 1:8, 1:4, 3:10] = gd[:, None, None] * gh[None, :, None] * gw[None, None, :]
    assert np.abs(got - want).max() <= S.ref_bound(x, sigmas_of(radii))
    assert np.array_equal(got != 0, want != 0)


def test_a_constant_volume_stays_constant_within_the_bound(ops):
    radii = (3, 1, 32)
    x = np.full((1, 6, 7, 37), 1234.5, np.float32)
    got = check(ops, x, radii)
    # the float32 taps of an axis sum to 1 within (2 r + 1) 2^-24; the sums themselves add the bound of `check`
    slack = sum(2 * r + 1 for r in radii) * U24 * 1234.5
    assert np.abs(got.astype(np.float64) - 1234.5).max() <= S.ref_bound(x, sigmas_of(radii)) + slack


def test_keep_zero_writes_plus_zero_and_leaves_the_rest(ops):
    radii = (3, 1, 3)
    x = volume((2, 9, 10, 21), 7)
    x[np.abs(x) < 1e-3] = 1.0
    x[:, 2:5] = 0.0
    x[:, :, :, 7:9] = 0.0
    x[0, 6, 3, 11] = -0.0
    x[1, 7, 5, 20] = 0.0                                    # a lone zero in the tail item of a row
    plain, kept = check(ops, x, radii), check(ops, x, radii, keep_zero=True)
    zero = x == 0
    assert zero[0, 6, 3, 11] and np.all(kept.view(np.uint32)[zero] == 0)           # +0.0f, bit for bit
    assert np.all(plain[zero] != 0)
    assert np.array_equal(kept.view(np.uint32)[~zero], plain.view(np.uint32)[~zero])


def test_a_nan_spreads_exactly_to_its_stencil_box(ops):
    for radii, at in (((3, 1, 3), (0, 4, 2, 6)), ((1, 0, 3), (1, 0, 3, 12)), ((0, 3, 0), (0, 1, 5, 3))):
        x = volume((2, 9, 7, 13), 9)
        x[at] = np.nan
        got = ops.prep_smooth(dev(x), sigmas_of(radii)).cpu().numpy()
        box = np.zeros(x.shape, bool)
        box[(at[0],) + tuple(slice(max(0, c - r), c + r + 1) for c, r in zip(at[1:], radii))] = True
        assert np.array_equal(np.isnan(got), box), radii
        want = S.ref_smooth(x, sigmas_of(radii)).astype(np.float32)
        assert np.abs(got[~box].astype(np.float64) - want[~box]).max() <= S.ref_bound(x, sigmas_of(radii))


def test_every_radius_zero_returns_the_input_itself_and_bad_sigmas_are_refused(ops):
    x = dev(volume((1, 4, 5, 6)))
    assert ops.prep_smooth(x, (0.0, 0.0, 0.0)) is x
    assert ops.prep_smooth(x, (0.1, 0.0, 0.05), True) is x                  # radii of 0: not filtered
    for bad in ((8.2, 0, 0), (-1.0, 0, 0), (float("nan"), 0, 0), (1.0, 1.0)):
        with pytest.raises(_lib.EffqError):
            ops.prep_smooth(x, bad)
    with pytest.raises(_lib.EffqError):
        ops.prep_smooth(x.to(torch.float64), (0.75, 0, 0))


def test_bad_arguments_are_refused_before_any_launch(ops):
    shape = (2, 4, 5, 6)
    n = int(np.prod(shape))
    x = dev(volume(shape))
    y, tmp = torch.full((n + 8,), 7.0, device=DEV), torch.full((n + 8,), 7.0, device=DEV)
    big = torch.zeros(2 * n, device=DEV)
    g = prep.antialias_taps(0.75)
    assert len(g) == 4
    wide = np.full(34, 1.0 / 67, np.float32)
    tp = g.ctypes.data
    good = dict(x=x.data_ptr(), dims=shape, td=tp, rd=3, th=tp, rh=3, tw=tp, rw=3, kz=0, y=y.data_ptr(), tmp=tmp.data_ptr())

    def call(**over):
        a = dict(good, **over)
        return ops.lib.effq_prep_smooth(a["x"], *a["dims"], a["td"], a["rd"], a["th"], a["rh"], a["tw"], a["rw"], a["kz"],
                                        a["y"], a["tmp"], ops.stream)
    bad = [dict(x=None), dict(y=None),
           dict(rd=-1), dict(rh=-1), dict(rw=-1),
           dict(rd=33, td=wide.ctypes.data), dict(rh=33, th=wide.ctypes.data), dict(rw=33, tw=wide.ctypes.data),
           dict(rd=0, rh=0, rw=0),                                             # nothing to do
           dict(tmp=None), dict(tmp=None, rd=0),                               # three and two filtered axes without tmp
           dict(y=x.data_ptr()), dict(tmp=x.data_ptr()), dict(tmp=y.data_ptr()),            # aliasing
           dict(x=big.data_ptr(), y=big.data_ptr() + 4 * (n - 1)),                          # overlapping by one voxel
           dict(x=big.data_ptr() + 4 * (n - 1), tmp=big.data_ptr()),
           dict(x=x.data_ptr() + 2), dict(y=y.data_ptr() + 1), dict(tmp=tmp.data_ptr() + 2),   # misaligned
           dict(dims=(0, 4, 5, 6)), dict(dims=(2, 0, 5, 6)), dict(dims=(2, 4, 5, 0)), dict(dims=(2, 4, 5, -6)),
           dict(dims=(1, 1, 1, 32768)), dict(dims=(1, 32768, 1, 1)), dict(dims=(3, 32767, 32767, 1)),   # 2^31 and more
           dict(td=None), dict(tw=None), dict(kz=2)]
    for over in bad:
        assert call(**over) == 1, over                                         # EFFQ_ERR_ARG
        assert b"argument check failed" in ops.lib.effq_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((tmp == 7.0).all())                 # nothing was launched
    # what is legal: one filtered axis without tmp, taps of an unfiltered axis null, x and y side by side in one buffer
    assert call(tmp=None, rd=0, rh=0, td=None, th=None) == _lib.EFFQ_OK
    assert call(x=big.data_ptr(), y=big.data_ptr() + 4 * n, tmp=None, rh=0, rw=0) == _lib.EFFQ_OK
    torch.cuda.synchronize()


# ---- end to end -----------------------------------------------------------------------------------------------------------
SOURCE, SPACING, TARGET = (40, 48, 56), (0.5, 1.25, 2.0), "1.25,1.75,2"      # factors 2.5, 1.4, 1: radii 3, 1, 0


def _lits_set(root):
    os.makedirs(os.path.join(root, "src"))
    aff = np.diag(SPACING + (1.0,))
    aff[:3, 3] = (-10.0, 4.0, 30.0)
    zz, yy, xx = np.meshgrid(*(np.arange(n) for n in SOURCE), indexing="ij")
    rows, truth = [], {}
    for k, sn in enumerate(("l1", "l2")):
        g = np.random.default_rng(60 + k)
        ct = (-500.0 + 18.0 * zz + 12.0 * yy - 9.0 * xx + 80.0 * g.standard_normal(SOURCE)).astype(np.int16)
        ct[5 + k, 7, 9] = 3000                                   # metal: clipped before it is smeared
        seg = ((zz - 20) ** 2 + (yy - 24) ** 2 + (xx - 28) ** 2 < 120 + 30 * k).astype(np.uint8) * 2
        R.write_scan(os.path.join(root, "src", f"{sn}_ct.nii.gz"), ct, affine=aff)
        R.write_scan(os.path.join(root, "src", f"{sn}_seg.nii.gz"), seg, affine=aff)
        rows.append([sn, f"src/{sn}_ct.nii.gz", f"src/{sn}_seg.nii.gz"])
        truth[sn] = (ct, seg)
    return R.write_list(os.path.join(root, "cases.csv"), rows, head=("subject", "ct", "seg")), truth


class Recorder:
    """The device ops with a record of the working arrays prep.process_subject ends with."""

    def __init__(self, ops):
        self._ops, self.arrays = ops, []

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def prep_standardise_crop(self, *a, **kw):
        y = self._ops.prep_standardise_crop(*a, **kw)
        self.arrays.append(y.cpu().numpy())
        return y


def test_prep_and_predict_missions_filter_on_the_device(ops, tmp_path, capsys):
    root = str(tmp_path)
    lst, truth = _lits_set(root)
    out = os.path.join(root, "data")
    entrance.main(["prep", "--task", "lits", "--src_list", lst, "--data_dir", out, "--prep_spacing", TARGET,
                   "--prep_antialias", "--prep_window", "-200,250", "--prep_min_size", "16,16,16"])
    said = capsys.readouterr().out
    factors = (2.5, 1.4, 1.0)
    sig = tuple(S.ref_sigma(f) for f in factors)
    assert sig == pytest.approx((0.75, 0.2, 0.0)) and tuple(S.ref_radius(s) for s in sig) == (3, 1, 0)
    grid =tuple(prep.resample_extent(n, f) for n, f in zip(SOURCE, factors))
    assert grid == (16, 34, 56)
    table = list(csv.DictReader(open(os.path.join(out, prep.PREP_CSV))))
    assert [r["subject"] for r in table] == ["l1", "l2"] and list(table[0])[-1] == "antialias"
    arrays = {}
    for r in table:
        sn = r["subject"]
        assert r["antialias"] == "0.75 0.2 0" and r["grid_shape"] == "16 34 56"
        assert f"{sn}: 40 48 56, anti-alias sigma 0.75 0.2 0 -> 16 34 56" in said
        x = np.clip(truth[sn][0].astype(np.float32), np.float32(-200), np.float32(250))[None]
        v = R.ref_resample_linear(S.ref_smooth(x, sig), factors, grid)                     # fp64 all the way
        mean, std = v.mean(), v.std()
        want = (v - mean) / std
        arr = arrays[sn] = np.load(os.path.join(out, "ct", f"{sn}.npy"))
        assert arr.shape == grid and arr.dtype == np.float32
        # e = the filter's bound plus the resampling's (test_prep_gpu.py: 8 2^-24 max |x|), max |x| = 250 after the window;
        # mean and std of the device's volume move by at most e each, then one float32 rounding
        e = S.ref_bound(x, sig) + 8 * U24 * 250.0
        assert S.ref_bound(x, sig) == (9 + 5) * U24 * 250.0
        tol = (2.0 + np.abs(want[0])) * e / std + np.spacing(np.abs(want[0]).astype(np.float32))
        err = np.abs(arr.astype(np.float64) - want[0])
        print(f"{sn}: max err {err.max():.3e}, least tolerance {tol.min():.3e}")
        assert np.all(err <= tol)
        plain = R.ref_resample_linear(x, factors, grid)
        assert np.abs((plain - plain.mean()) / plain.std() - want).max() > 100 * tol.max()   # the filter did its work
        assert np.array_equal(np.load(os.path.join(out, "seg", f"{sn}.npy")),
                              R.ref_resample_nearest(truth[sn][1][None], factors, grid)[0])  # the label is not touched

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
                     prep_antialias=True, prep_window="-200,250", merge_type=None).items():
        setattr(args, k, v)
    rec = Recorder(ops)
    rows = predict.run(args, ops=rec, model=model, window_batch=8)
    said = capsys.readouterr().out
    assert [r["subject"] for r in rows] == ["l1", "l2"] and len(rec.arrays) == 2
    for r, y in zip(rows, rec.arrays):
        assert np.array_equal(y[0].view(np.uint32), arrays[r["subject"]].view(np.uint32))
        assert f"{r['subject']}: 40 48 56, anti-alias sigma 0.75 0.2 0 -> grid 16 34 56" in said
    table = list(csv.reader(open(os.path.join(seg, predict.PREDICT_CSV))))
    assert table[0] == predict.CSV_HEADER + ["antialias"] and [r[-1] for r in table[1:]] == ["0.75 0.2 0"] * 2
    assert sorted(os.listdir(seg)) == ["l1.nii.gz", "l2.nii.gz", "predict.csv"]
