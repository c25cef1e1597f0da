"""The kernels of --prep_denoise nlmM against the fp64 restatement, and the whole filter on a phantom.

The bound, per voxel of Omega:  |y - y_ref| <= K(M) 2^-24 spread + 2^-24 |y_ref| (the one rounding of y),  spread = max -
min of the finite v in the voxel's search window.  Derivation, with eps = 2^-24, N = (2M + 1)^3 - 1
candidates, a_j the exponent of candidate j and w_j = exp(-a_j):
  * d2 is a sum of 27 non-negative fp32 terms: relative error at most 30 eps, so |da_j| <= 30 eps (a_j + 2 / H2); exp2
    adds 1 ulp = 2 eps: the relative error of w_j is at most eps (30 (a_j + 2) + 2).
  * The device forms y = v_i + sum w_j (v_j - v_i) / (sum w_j + wmax), the rule's quotient with v_i taken out; every
    |v_j - v_i| and |v_j - y| is at most spread.  A relative change of the weights moves y by at most spread times
    sum p_j |dw_j / w_j| + |dwmax / wmax| wmax / (sum w + wmax),  p_j = w_j / (sum w + wmax).  sum p_j (a_j + 2) <= amin + 2
    + sum p_j (a_j - amin), and that sum is -sum p_j ln(p_j Z), Z = (sum w + wmax) / wmax >= 1: at most the entropy of
    N + 1 outcomes, ln(N + 1).  The second term is at most (amin + 2) / 2.  fp32 weights are used only while wmax >=
    2^-16, amin <= A = 11.1 (a voxel below that is done in fp64): the weights cost 30 (1.5 (A + 2) + ln(N + 1)) + 3.
  * num takes N multiply-adds of rounded differences, den N additions, in fp32 in a fixed order: 2 N + 2; the sum
    with wmax and the division 2 more; 4 for what first order leaves out.
  K(M) = 30 (1.5 * 13.1 + ln(N + 1)) + 3 + 2 N + 8:  752 at M = 1, 1460 at M = 3, 3476 at M = 5."""
import math

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, denoise as N, ops_denoise as O, prep
from efficientq_amd.hip_ops import get_ops
from tests import prep_denoise_ref as R

pytestmark = pytest.mark.gpu
EPS32, (TD, TH, TW) = 2.0 ** -24, _lib.PREP_DENOISE_TILE
# rmse after / rmse before of the restatement on phantom() at nlm3, against the clean phantom
RECOVERY_MEASURED = 0.10268124


def K(radius):
    n = (2 * radius + 1) ** 3 - 1
    return 30.0 * (1.5 * 13.1 + math.log(n + 1)) + 3 + 2 * n + 8


@pytest.fixture(scope="module")
def ops():
    return get_ops("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def scan(shape):
    """300 + 200 * step + N(0, 20): a step along h and one along w, a slab of exact zeros, and NaN, +Inf, -0.0 and two
    negatives scattered in."""
    g = np.random.default_rng(sum(shape))
    d, h, w = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    v = (300.0 + 200.0 * ((h >= shape[1] // 2) + 1.0 * (w >= (2 * shape[2]) // 3)) + 20.0 * g.standard_normal(shape))
    v = v.astype(np.float32)
    v[:, :, shape[2] // 4] = 0.0
    flat = v.reshape(-1)
    flat[g.choice(flat.size, 5, replace=False)] = np.float32([np.nan, np.inf, -0.0, -50.0, -420.0])
    return v


def phantom():
    g = np.random.default_rng(5)
    clean = np.full((24, 24, 24), 300.0)
    clean[:, 8:, :] = 500.0
    clean[:, :, 14:] = 800.0
    clean[:4] = 0.0
    return clean, np.where(clean != 0, clean + 20.0 * g.standard_normal(clean.shape), 0.0).astype(np.float32)


def reference(v, mask, radius):
    """The restatement of one case: (r, sigma, n, y, spread, sumsq, count)."""
    r = R.residual(v, mask)
    s, n = R.sigma_of(r)
    s = s if n else 20.0                                              # a volume without an interior has no residual
    return (r, s, n) + R.nlm(v, mask, radius, s)


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def check_filter(v, mask, radius, got, want):
    """Assertions 2, 3 and 4 of one call: `got` = (y, sumsq, count) of the device, `want` of reference()."""
    y, sumsq, count = got
    _, _, _, y_ref, spread, sumsq_ref, count_ref = want
    om, y = R.omega(v, mask), y.cpu().numpy()
    assert np.array_equal(y.view(np.uint32)[~om], v.view(np.uint32)[~om])
    bound = K(radius) * EPS32 * spread + EPS32 * np.abs(y_ref)
    err, bound = np.abs(y[om].astype(np.float64) - y_ref[om]), bound[om]
    print(f"{v.shape} {mask} nlm{radius}: largest error / bound {np.max(err / np.maximum(bound, 1e-300), initial=0.0):.3g}")
    assert np.all(err <= bound)
    assert count == count_ref == int(om.sum())
    assert abs(sumsq - sumsq_ref) <= (2 * np.abs(y_ref[om] - v[om]) * bound + bound ** 2).sum() + 1e-12 * sumsq_ref


@pytest.mark.parametrize("shape, radius, mask", [
    ((2, 3, 4), 3, "nonzero"), ((TD + 1, 5, 6), 3, "nonzero"), ((5, TH + 1, 6), 3, "nonzero"), ((TD + 1, 5, 6), 3, "all"),
    ((5, 6, 2 * TW + 3), 3, "nonzero"), ((5, 6, 2 * TW + 3), 1, "nonzero"), ((5, 6, 2 * TW + 3), 5, "nonzero")])
def test_residuals_and_filter_against_the_restatement(ops, shape, radius, mask):
    v = scan(shape)
    want = reference(v, mask, radius)
    r_ref, sigma, n_ref = want[:3]
    assert np.array_equal(bits(O.prep_denoise_residual(ops, dev(v), mask)), r_ref.view(np.uint32))
    if n_ref >= N.MIN_SAMPLES:
        assert N.noise_sigma(ops, "s", "m", dev(v), mask) == (sigma, n_ref)
    else:
        with pytest.raises(prep.PrepError, match=f"subject s: modality m: --prep_denoise: {n_ref} residuals"):
            N.denoise(ops, "s", "m", dev(v), mask, radius)
    got = O.prep_denoise_nlm(ops, dev(v), mask, radius, sigma)
    check_filter(v, mask, radius, got, want)
    again = O.prep_denoise_nlm(ops, dev(v), mask, radius, sigma)
    assert np.array_equal(bits(got[0]), bits(again[0])) and got[1:] == again[1:]


def test_a_tiny_sigma_leaves_omega_as_it_came_and_a_constant_volume_stays(ops):
    v = scan((5, 6, 2 * TW + 3))
    sigma = 1e-6 * float(np.std(v[np.isfinite(v)], dtype=np.float64))           # sigma^2 = 1e-12 of the variance
    y, sumsq, count = O.prep_denoise_nlm(ops, dev(v), "nonzero", 3, sigma)
    assert np.array_equal(bits(y), v.view(np.uint32)) and sumsq == 0.0 and count == int(R.omega(v).sum())
    c = np.full((TD + 1, 5, 6), 3.7, dtype=np.float32)
    y, sumsq, count = O.prep_denoise_nlm(ops, dev(c), "all", 3, 1.0)
    assert np.all(np.abs(y.cpu().numpy().astype(np.float64) - c) <= 2 * np.spacing(c)) and count == c.size
    assert sumsq <= c.size * (2 * float(np.spacing(c[0, 0, 0]))) ** 2


def test_the_phantom_through_denoise(ops):
    clean, v = phantom()
    want = reference(v, "nonzero", 3)
    _, sigma, n, y_ref = want[:4]
    y, done = N.denoise(ops, "s", "m", dev(v), "nonzero", 3)
    assert (done.radius, done.sigma, done.samples) == (3, sigma, n)
    sumsq = done.rms ** 2 * want[6]
    check_filter(v, "nonzero", 3, (y, sumsq, want[6]), want)
    m, bound = clean != 0, K(3) * EPS32 * want[4] + EPS32 * np.abs(y_ref)
    rmse = lambda a: float(np.sqrt(((a.astype(np.float64) - clean)[m] ** 2).mean()))
    before, after_ref, after = rmse(v), rmse(y_ref), rmse(y.cpu().numpy())
    assert abs(after_ref / before - RECOVERY_MEASURED) <= 1e-7 and after_ref / before < 0.25
    assert after / before <= RECOVERY_MEASURED + 1e-7 + float(np.sqrt((bound[m] ** 2).mean())) / before
    assert abs(done.rms - sigma) < 0.25 * sigma and np.array_equal(bits(y)[~m], v.view(np.uint32)[~m])
