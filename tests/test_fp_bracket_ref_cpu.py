"""tests/fp_bracket_ref.py, the integer restatement of the bracketed activation-scale fit that
tests/test_fp_bracket_classes_gpu.py holds the kernel to, checked without a GPU: iterated on its own it ends where
oracle.effq_oracle.fit_scale ends, its fp64 sums lie inside the rounding bound of the exact ones, and the undecided set
shrinks with the bracket - the monotonicity the check of the compacted lists relies on.  Largest relative difference of
alpha to the oracle over the cases below: 2.9e-16 (bar 1e-11), 5 to 577 iterations, the same count in every case."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import fp_bracket_ref as R
from oracle import effq_oracle as O

# (name, tensor, levels, lo, hi): the inputs of the class tests
CASES = [("relu", R.relu(20011), L, 0.0, 1.0) for L in (2, 4, 16, 256)] + [
    ("relu8193", R.relu(8193), 256, 0.0, 1.0),
    ("signed", R.signed(16389), 16, -1.0, 1.0),
    ("bimodal", R.bimodal(12289), 8, 0.0, 1.0),
    ("bimodal", R.bimodal(12289), 16, 0.0, 1.0),
    ("five", R.five_valued(12289), 4, 0.0, 1.0),
    ("adversarial", R.adversarial(4), 4, 0.0, 1.0),
    ("tiny", R.relu(37), 4, 0.0, 1.0),
]


def test_the_yardstick_iterated_ends_where_the_oracle_ends():
    worst = 0.0
    print()
    for name, v, L, lo, hi in CASES:
        got = R.iterate(v, L, lo, hi)
        fit = O.fit_scale(torch.from_numpy(v), L, lo, hi)
        rel = abs(got["alpha"] - fit.alpha) / abs(fit.alpha)
        print(f"{name} n={v.size} L={L}: {got['it']} iterations, alpha rel diff {rel:.2e}")
        assert got["done"] == 1 and got["it"] == fit.iters, (name, L, got["it"], fit.iters)
        assert rel <= 1e-11, (name, L, rel)
        worst = max(worst, rel)
    print(f"largest relative difference of alpha to the oracle over {len(CASES)} cases: {worst:.2e} (bar 1e-11)")


def test_adversarial_values_straddle_the_boundaries_of_the_scales_they_are_classified_at():
    """At each of the first ADVERSARIAL_SCALES classification scales of the adversarial tensor's own fit, the tensor holds the
    fp32 value nearest to every level boundary and its two neighbours, and the neighbours lie on different levels: the
    values one ulp apart that the fp32 screen of the kernels cannot tell apart."""
    L, d = 4, 1.0 / 3.0
    v = R.adversarial(L)
    fit = R.iterate(v, L, 0.0, 1.0)
    assert fit["it"] > R.ADVERSARIAL_SCALES
    assert fit["alphas"][0] == math.fsum(np.abs(v.astype(np.float64)).tolist()) / v.size
    bits = v.view(np.uint32)
    for j in range(R.ADVERSARIAL_SCALES):
        a = fit["alphas"][j]
        tr = R.boundary_triples(a, L)
        assert np.isin(tr.view(np.uint32), bits).all(), j
        lv = R.level(tr.astype(np.float64), a, 0.0, 1.0, d)
        assert lv[0].tolist() == [0, 1, 2] and lv[2].tolist() == [1, 2, 3], (j, lv.tolist())
        assert all(lv[1][k] in (k, k + 1) for k in range(L - 1))
        # within an ulp of fp32 of the boundary: the screen's own error (1.5 lmax 2^-24) is larger than that
        t = tr.astype(np.float64) / a / d
        assert np.abs(t - (np.arange(1, L) - 0.5)).max() <= 3 * 2.0 ** -23 * (L - 0.5)
    # the rest of what the case is there for
    assert (v == np.float32(1e-42)).sum() == 30 and (v == np.float32(1e-30)).sum() == 30
    assert (np.signbit(v) & (v == 0.0)).sum() == 20 and (v < 0.0).sum() == 30


def test_unit_exponent_leaves_no_room_for_overflow():
    assert R.unit_exponent(4, 1000.0) == 60 - 11                                   # 3000 = 1.46 * 2^11
    assert R.unit_exponent(2, 1.0) == 60 and R.unit_exponent(2, 0.75) == 61
    assert R.unit_exponent(4, 0.0) == 0 and R.unit_exponent(4, math.inf) == 0 and R.unit_exponent(4, 1e-320) == 1000
    for name, v, L, lo, hi in CASES:
        s = math.fsum(np.abs(v.astype(np.float64)))
        e = R.unit_exponent(L, s)
        u = R.units(v, e)
        assert (L - 1) * sum(abs(int(x)) for x in u) < 2 ** 61 + (L - 1) * v.size
        # rounding to the unit moves no value by more than half a unit
        err = np.abs(np.ldexp(u.astype(np.float64), -e) - v.astype(np.float64))
        assert err.max() <= math.ldexp(0.5, -e)
    assert R.units(np.array([0.5, 1.5, 2.5, -0.5, -1.5], np.float32), 0).tolist() == [0, 2, 2, 0, -2]   # half to even


def test_fp64_sums_lie_inside_the_rounding_bound_of_the_exact_ones():
    worst = [0.0, 0.0]
    for name, v, L, lo, hi in CASES:
        d = (hi - lo) / (L - 1)
        fit = R.iterate(v, L, lo, hi)
        u, q, x = R.units(v, fit["e"]), math.ldexp(1.0, -fit["e"]), v.astype(np.float64)
        for a in fit["alphas"][:3] + fit["alphas"][-2:]:
            t = R.tallies(x, u, a, lo, hi, d)
            f, exact, absolute = R.sums_from_tallies(t, v.size, lo, d, q)
            for i, k in ((0, 4), (1, 8)):
                assert R.within(f[i], exact[i], absolute[i], k), (name, L, i)
                worst[i] = max(worst[i], float(abs(Fraction(f[i]) - exact[i]) / absolute[i]) / R.U53)
            # the exact sums ARE the sums over the values: sum b u q with b = l d + lo, term by term
            l = R.level(x, a, lo, hi, d)
            D, LO = Fraction(d), Fraction(lo)
            assert exact[0] == Fraction(q) * (D * int((l * u).sum()) + LO * int(u.sum()))
            assert exact[1] == D * D * int((l * l).sum()) + 2 * D * LO * int(l.sum()) + LO * LO * v.size
    print(f"\nworst error of the fp64 sums, in roundings of the absolute terms: {worst[0]:.2f} (of 4), {worst[1]:.2f} (of 8)")
    assert not R.within(math.nan, Fraction(1), Fraction(1), 4) and not R.within(1.0 + 8 * R.U53, Fraction(1), Fraction(1), 4)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-L{c[2]}")
def test_undecided_shrinks_with_the_bracket(case):
    name, v, L, lo, hi = case
    d = (hi - lo) / (L - 1)
    x = v.astype(np.float64)
    a = R.iterate(v, L, lo, hi)["alpha"]
    rng = np.random.default_rng(7)
    strict = 0
    for _ in range(40):
        w = a * 10.0 ** rng.uniform(-6, 0.5)
        olo, ohi = a - w * rng.uniform(0, 1), a + w * rng.uniform(0, 1)
        ilo, ihi = sorted(rng.uniform(olo, ohi, 2))
        if rng.integers(0, 4) == 0:
            olo, ohi = (1e-300, 1e300) if lo == 0.0 else (0.0, math.inf)               # the brackets of the two bases
        if not (olo >= 0.0 and ilo > 0.0):
            continue
        outer, inner = R.undecided(x, olo, ohi, lo, hi, d), R.undecided(x, ilo, ihi, lo, hi, d)
        assert not (inner & ~outer).any(), (olo, ilo, ihi, ohi)
        strict += int(outer.sum() > inner.sum())
        # a decided value has ONE level inside the bracket: at both ends and at a scale in between
        mid = 0.5 * (ilo + ihi)
        dec = ~inner
        assert np.array_equal(R.level(x[dec], mid, lo, hi, d), R.level(x[dec], ilo, lo, hi, d))
    assert strict >= 5


def test_the_base_of_a_post_relu_fit_lists_exactly_the_positive_values():
    v = R.adversarial(4)
    und = R.undecided(v.astype(np.float64), 1e-300, 1e300, 0.0, 1.0, 1.0 / 3.0)
    assert np.array_equal(und, v > 0.0)                     # zeros of either sign and negatives: one level at every scale
    assert und[v == np.float32(1e-42)].all() and und[v == np.float32(1e-30)].all()


def test_shape_is_fbr_shapes():
    assert R.shape(3) == (1, 4) and R.shape(37) == (1, 40) and R.shape(8192) == (1, 8192) and R.shape(8193) == (2, 4100)
    assert R.shape(20011) == (3, 6672) and R.shape(8 * 2 ** 20 + 5) == (1024, 8196)
    n = 8 * 2 ** 20 + 5
    assert 0 < n - 1023 * 8196 < 8196                       # a short last slice
