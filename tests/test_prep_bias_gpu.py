"""The kernels of --prep_bias n4 against the fp64 restatement, and the whole correction on a phantom."""
import numpy as np
import pytest
import torch

from efficientq_amd import bias as B, ops_bias as O
from efficientq_amd.hip_ops import get_ops
from tests import prep_bias_backend as K, prep_bias_ref as R

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -24                     # the relative error of one rounding to fp32
# the restatement's own deviation from the true field of R.phantom(), normalised to mean 1 over M
RECOVERY_MEASURED = 0.04692770707573879


@pytest.fixture(scope="module")
def ops():
    return get_ops("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def scan(shape, seed):
    """A positive scan with zeros, negatives, NaN and Inf outside M, and the first quarter of axis 0 outside M: at levels
    2 and 3 the control points that only those planes reach get no sample."""
    g = np.random.default_rng(seed)
    v = (200.0 + 800.0 * g.random(shape)).astype(np.float32)
    v[:-(-shape[0] // 4)] = 0.0
    flat = v.reshape(-1)
    flat[g.choice(flat.size, 40, replace=False)] = np.repeat(np.float32([np.nan, np.inf, -3.0, 0.0]), 10)
    return v


# 13 x 10 x 21: stride 1;  37 x 33 x 45: stride 4 with ragged ends;  12 x 40 x 37: mixed strides;  9 x 140 x 33: two slabs
# per plane (35 sampled rows);  9 x 33 x 262: two chunks of W (65 samples)
@pytest.mark.parametrize("shape", [(13, 10, 21), (37, 33, 45), (12, 40, 37), (9, 140, 33), (9, 33, 262)])
def test_histogram_and_fit_against_the_restatement_at_every_level(ops, shape):
    """Bounds.  The device forms e in fp64 by the restatement's own operations and rounds it to fp32 once, |de| <= 2^-24 |e|;
    every sum after that is fp64.  So |dphi_c| <= 2^-24 phi_c(|e|), the lattice of |e|, plus fp64 summation error (1e-12
    of it is generous).  The weights of a sample sum to 1, so eval(phi) moves by at most max_c |dphi_c|; f = fp32(f +
    fp32(df)) adds two roundings, 2^-24 (|df| + |f + df|).  The two sums are formed from the fp64 df of the device's own
    phi: against exp of the restatement's evaluation of that phi they differ by the order of fp64 sums only, 1e-13."""
    v = scan(shape, sum(shape))
    stride, offset = zip(*(B.sample_rule(n) for n in shape))
    u, m = O.prep_bias_log(ops, dev(v))
    want_u, want_m = R.log_mask(v)
    assert np.array_equal(m.cpu().numpy() != 0, want_m) and np.allclose(u.cpu().numpy(), want_u, rtol=2 * EPS32, atol=0)
    idx = [np.arange(o, n, s) for n, s, o in zip(shape, stride, offset)]
    grid = np.ix_(*idx)
    u_s, m_s = u.cpu().numpy()[grid], want_m[grid]
    g = np.random.default_rng(1)
    f0 = (0.05 * g.standard_normal(u_s.shape)).astype(np.float32)
    counters, lo, hi, n = O.prep_bias_hist(ops, u, m, dev(f0), stride, offset)
    want_h, want_lo, want_hi = R.histogram((u_s - f0)[m_s])
    assert (lo, hi, n) == (want_lo, want_hi, int(m_s.sum())) and np.array_equal(counters, want_h)
    table = R.sharpen(want_h / 65536.0, lo, hi)
    zeros = 0
    for level in range(R.LEVELS):
        axes = [R.dense_weights(size, level, i) for size, i in zip(shape, idx)]
        cells = (2 ** level + 3) ** 3
        before = g.standard_normal(cells)
        runs = []
        for _ in range(2):
            f, phi, lat = dev(f0), torch.empty(cells, dtype=torch.float64, device="cuda:0"), dev(before)
            sums = O.prep_bias_fit(ops, u, m, f, stride, offset, level, lo, hi, table, phi, lat)
            runs.append((phi.cpu().numpy(), lat.cpu().numpy(), f.cpu().numpy(), np.float64(sums)))
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(*runs))
        got_phi, got_lat, got_f, got_sums = runs[0]
        e, want_phi, df, _, _ = R.fit_step(u_s, f0, m_s, table, lo, hi, axes)
        tol = (EPS32 + 1e-12) * R.lattice(np.abs(e), m_s, axes).reshape(-1)
        empty = want_phi.reshape(-1) == 0
        zeros += int(empty.sum())
        assert np.all(np.abs(got_phi - want_phi.reshape(-1)) <= tol) and np.all(got_phi[empty] == 0)
        assert np.all(np.abs(got_lat - (before + want_phi.reshape(-1))) <= tol + 2.0 ** -52 * np.abs(got_lat))
        want_f = f0.astype(np.float64) + df
        f_tol = tol.max() + EPS32 * (np.abs(df) + np.abs(want_f)) + 1e-30
        assert np.all(np.abs(got_f - want_f) <= f_tol)
        x = np.exp(R.evaluate(got_phi.reshape(want_phi.shape), axes)[m_s])
        assert np.all(np.abs(got_sums - [x.sum(), (x * x).sum()]) <= 1e-13 * np.float64([x.sum(), (x * x).sum()]))
    assert zeros > 0


def hist_case(name):
    g = np.random.default_rng(2)
    if name == "centres":                # every value a bin centre of [0, 199], both ends among them: no fraction
        return g.permutation(np.tile(np.arange(200, dtype=np.float32), 3)).reshape(6, 10, 10)
    if name == "one":                    # one sample
        return np.float32([[[0.25]]])
    if name == "constant":               # min == max: reported, nothing counted
        return np.full((5, 6, 7), 1.5, dtype=np.float32)
    u = np.full((48, 48, 32), 57.0, dtype=np.float32)       # 73726 samples on one centre: more than 2^16 in one bin
    u[0, 0, 0], u[-1, -1, -1] = 0.0, 199.0
    return u


@pytest.mark.parametrize("name", ["centres", "one", "constant", "many"])
def test_histogram_counters_equal_the_restatement(ops, name):
    u = hist_case(name)
    m, f = np.ones(u.shape, dtype=np.uint8), np.zeros(u.shape, dtype=np.float32)
    counters, lo, hi, n = O.prep_bias_hist(ops, dev(u), dev(m), dev(f), (1, 1, 1), (0, 0, 0))
    want, want_lo, want_hi = R.histogram(u.reshape(-1))
    assert (lo, hi, n) == (want_lo, want_hi, u.size) and np.array_equal(counters, want)
    if name in ("one", "constant"):
        assert lo == hi and not counters.any()
    else:
        assert counters.sum() == u.size * 65536 and not (counters % 65536).any()
        assert counters[57] >= 2 ** 32 or name == "centres"


@pytest.mark.parametrize("shape", [(5, 7, 67), (3, 4, 130), (6, 5, 3)])
def test_apply_divides_the_full_grid_by_the_field(ops, shape):
    """Against fp64 rounded to fp32: equal, or one ulp apart where the device's fp64 exp and numpy's differ in the last
    bit and the quotient lies on a rounding boundary (measured: DESIGN section 30)."""
    g = np.random.default_rng(sum(shape))
    v = scan(shape, 7)
    lattices = 0.1 * g.standard_normal(O.LATTICE)
    m = R.log_mask(v)[1].astype(np.uint8)
    y, lo, hi = O.prep_bias_apply(ops, dev(v), dev(m), dev(lattices))
    want, want_lo, want_hi = K.BiasMixin().prep_bias_apply(torch.from_numpy(v), torch.from_numpy(m), torch.from_numpy(lattices))
    got, want = y.cpu().numpy(), want.numpy()
    finite = np.isfinite(v)
    ulps = np.abs(got[finite].view(np.int32).astype(np.int64) - want[finite].view(np.int32).astype(np.int64))
    assert ulps.max() <= 1
    assert np.array_equal(got[~finite].view(np.int32), v[~finite].view(np.int32))          # NaN and Inf as they were
    assert np.all(got[v == 0] == 0) and np.all(got[v < 0] < 0)
    assert abs(lo - want_lo) <= 2 * EPS32 * want_lo and abs(hi - want_hi) <= 2 * EPS32 * want_hi


def test_recovery_of_a_known_field_on_the_device(ops):
    v, field, tissue = R.phantom()
    _, want_iters, _ = R.correct(v)
    y, done = B.correct(ops, "phantom", "t1", dev(v))
    y = y.cpu().numpy().astype(np.float64)
    m = v > 0
    got = np.where(m, v / np.where(m, y, 1.0), 1.0)              # exp(f), from what the device wrote
    deviation = np.abs(got[m] / got[m].mean() - field[m] / field[m].mean()).max()
    assert list(done.iters) == want_iters and deviation <= 2 * RECOVERY_MEASURED
    for k in (1, 2, 3):
        a, b = v[tissue == k].astype(np.float64), y[tissue == k]
        assert b.std() / b.mean() < a.std() / a.mean()
