"""The arithmetic of the bracketed activation-scale fit (csrc/fixed_point_bracket.hip) restated with numpy and Python
integers (tests/test_fp_bracket_ref_cpu.py, tests/test_fp_bracket_classes_gpu.py).  No GPU, no library.

A restatement of WHAT a pass must add up, not of the planner that decides which values a pass reads: whatever the
bracket, the source list and the pass class, "decided tallies + undecided list = the whole tensor" has to give

  unit_exponent      the exponent e of the integer unit q = 2^-e, as k_fbr_init chooses it from sum |v|;
  units              u = rint(v 2^e): the product is exact in fp64 and rounds half to even;
  level              the reference's level index rint((clamp(v / a) - lo) / d) in fp64 (level_exact of csrc/fp_level.h);
  tallies            (sum l u, sum l, sum l^2, sum u) as Python integers;
  undecided          the values whose level differs between the two ends of a bracket;
  sums_from_tallies  the two sums of the scale update from four tallies: in fp64 in the kernel's order of operations, and
                     exactly (fractions.Fraction), with the sum of the absolute terms a rounding bound is taken from.

The constants of k_fbr_init and fbr_shape are literals here on purpose: a retuned kernel then fails the tests instead of
being followed by them."""
import functools
import math
from fractions import Fraction

import numpy as np

MIN_PER = 8192                   # FBR_MIN_PER: values per workgroup below which fewer workgroups are used
MAXG = 1024                      # FBR_MAXG
U53 = 2.0 ** -53                 # one rounding of an fp64 operation, relative


def shape(n):
    """(G, per) of fbr_shape: workgroups, values per slice (a multiple of 4)."""
    g = min(max((n + MIN_PER - 1) // MIN_PER, 1), MAXG)
    return g, ((n + g - 1) // g + 3) & ~3


def unit_exponent(levels, sum_abs):
    """e with (levels - 1) * sum|v| * 2^e < 2^61: no partial sum of level * u can overflow 63 bits."""
    bound = float(levels - 1) * float(sum_abs)
    e = 0
    if 0.0 < bound < 1e300:
        e = 60 - (math.frexp(bound)[1] - 1)          # ilogb
    return max(min(e, 1000), -1000)


def units(v, e):
    """rint(v * 2^e) as int64: scaling by a power of two is exact, numpy's rint rounds half to even."""
    x = np.ascontiguousarray(v, dtype=np.float32).reshape(-1).astype(np.float64)
    return np.rint(np.ldexp(x, e)).astype(np.int64)


def level(v, a, lo, hi, d):
    """level_exact of csrc/fp_level.h as int64: IEEE fp64 division, C's fmin / fmax (they drop a NaN operand), subtraction,
    division, round half to even."""
    with np.errstate(all="ignore"):
        t = np.asarray(v, dtype=np.float64) / np.float64(a)
        t = np.fmin(np.fmax(t, lo), hi)
        return np.rint((t - lo) / d).astype(np.int64)


def tallies(v, u, a, lo, hi, d, mask=None):
    """(sum l u, sum l, sum l^2, sum u) over the values of `mask` (all of them if None) at scale a, as Python integers.
    The int64 sums cannot wrap: |sum l u| <= (levels - 1) sum |u| < 2^61 + n by the choice of the unit."""
    if mask is not None:
        v, u = v[mask], u[mask]
    l = level(v, a, lo, hi, d)
    assert float(l.max(initial=0)) * float(np.abs(u).astype(np.float64).sum()) < 2.0 ** 62
    return (int((l * u).sum()), int(l.sum()), int((l * l).sum()), int(u.sum()))


def undecided(v, blo, bhi, lo, hi, d):
    """Boolean mask: the level at the lower end of the bracket differs from the level at its upper end.  The level is
    monotone in the scale, so everywhere else it is the same for every scale of the bracket."""
    return level(v, blo, lo, hi, d) != level(v, bhi, lo, hi, d)


def sums_from_tallies(t, n, lo, d, q):
    """[sum b v, sum b b] of b = l d + lo from the tallies t, in the unit q:
         sum b v = d q t0 + lo q t3,       sum b b = d^2 t2 + 2 d lo t1 + lo^2 n.
    Returns (fp64, exact, absolute): the pair in fp64 in k_fbr_finish's order of operations, the pair as Fractions of the
    fp64 constants d, lo, q, and per sum the sum of the absolute values of its terms."""
    t0, t1, t2, t3 = (int(x) for x in t)
    d, lo, q = float(d), float(lo), float(q)
    srx, sx = q * float(t0), q * float(t3)
    f0 = d * srx + lo * sx
    f1 = (d * d * float(t2) + 2.0 * d * lo * float(t1)) + lo * lo * float(n)
    D, LO, Q = Fraction(d), Fraction(lo), Fraction(q)
    terms0 = (D * Q * t0, LO * Q * t3)
    terms1 = (D * D * t2, 2 * D * LO * t1, LO * LO * n)
    return (f0, f1), (sum(terms0), sum(terms1)), (sum(abs(x) for x in terms0), sum(abs(x) for x in terms1))


def within(got, exact, absolute, roundings):
    """|got - exact| <= roundings * 2^-53 * absolute, evaluated exactly; a got that is not finite fails."""
    if not math.isfinite(got):
        return False
    return abs(Fraction(got) - exact) <= Fraction(roundings) * Fraction(U53) * absolute


def stop(it, max_iter, a_new, alpha, tol):
    """fp_stop of csrc/fp_level.h: 2 at the cap (even where the last step converged), 1 once the step is within tol (or
    NaN), else 0."""
    if it >= max_iter:
        return 2
    return 0 if abs(a_new - alpha) > tol else 1


def iterate(v, levels, lo, hi, tol=1e-5, max_iter=None):
    """The fit by the yardstick alone: every pass tallies the WHOLE tensor at the current scale.  dict(alpha, it, done,
    alphas = the classification scales, e)."""
    x = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    n = x.size
    max_iter = 100 * levels if max_iter is None else max_iter
    d = (hi - lo) / (levels - 1)
    sum_abs = math.fsum(np.abs(x.astype(np.float64)))
    e = unit_exponent(levels, sum_abs)
    u, q = units(x, e), math.ldexp(1.0, -e)
    x64 = x.astype(np.float64)
    a, alphas, it, done = sum_abs / float(n), [], 0, 0
    while not done:
        alphas.append(a)
        (s0, s1), _, _ = sums_from_tallies(tallies(x64, u, a, lo, hi, d), n, lo, d, q)
        a_new = s0 / s1
        it += 1
        done = stop(it, max_iter, a_new, a, tol)
        a = a_new
    return {"alpha": a, "it": it, "done": done, "alphas": alphas, "e": e}


def ulp_shift(x, k):
    """The fp32 values k units in the last place above (k < 0: below) x."""
    i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    m = np.where(i >= 0, i, -(i & 0x7FFFFFFF)) + int(k)
    return np.where(m >= 0, m, (-m) | 0x80000000).astype(np.uint32).view(np.float32)


# ---- the inputs of the class tests: small tensors that reach every pass class of the kernel ---------------------------
def relu(n, seed=125):
    rng = np.random.default_rng(seed)
    return np.maximum(rng.standard_normal(n) * 1.7 + 0.2, 0.0).astype(np.float32)


def signed(n, seed=124):
    return (np.random.default_rng(seed).standard_normal(n) * 0.3 + 0.05).astype(np.float32)


def bimodal(n, seed=125):
    rng = np.random.default_rng(seed)
    h = n // 2
    x = np.concatenate([rng.standard_normal(h) * 0.05 + 0.2, rng.standard_normal(n - h) * 0.3 + 3.0])
    return np.maximum(x, 0.0).astype(np.float32)


def five_valued(n, seed=126):
    rng = np.random.default_rng(seed)
    return np.array([0.0, 0.3, 0.93, 1.13, 2.93], np.float32)[rng.choice(5, n, p=[0.28, 0.31, 0.10, 0.25, 0.06])]


ADVERSARIAL_SCALES = 3           # classification scales of the adversarial tensor that have values on their boundaries


def boundary_triples(a, levels, lo=0.0, hi=1.0):
    """[3][levels - 1] fp32: the values one ulp below, ON (to fp32) and one ulp above the level boundaries (k - 0.5) d + lo
    of the scale a.  At a the row below has the levels 0 .. levels - 2 and the row above 1 .. levels - 1; the middle row
    falls to whichever side its rounding to fp32 went."""
    d = (hi - lo) / (levels - 1)
    p = (((np.arange(1, levels) - 0.5) * d + lo) * a).astype(np.float32)
    return np.stack([ulp_shift(p, -1), p, ulp_shift(p, 1)])


@functools.lru_cache(maxsize=None)
def _adversarial(levels, seed):
    f32 = np.float32
    fixed = [relu(20011, seed), np.full(30, 1e-30, f32), np.full(30, 1e-42, f32), -np.zeros(20, f32),
             np.full(25, -0.3, f32), np.full(5, -1e-30, f32)]

    def build(scales, a0):
        v = np.concatenate(fixed + [np.tile(boundary_triples(a, levels).reshape(-1), 2) for a in scales])
        s = math.fsum(np.abs(v.astype(np.float64)).tolist())
        if a0 is None:
            return None, (s + 3.0) / (v.size + 1)
        return np.concatenate([v, [a0 * (v.size + 1) - s]]).astype(f32), a0

    alphas = iterate(np.concatenate(fixed), levels, 0.0, 1.0)["alphas"]
    assert len(alphas) > ADVERSARIAL_SCALES
    _, a0 = build(alphas[:ADVERSARIAL_SCALES], None)
    v = None
    for _ in range(16):
        nv, _ = build([a0] + alphas[1:ADVERSARIAL_SCALES], a0)
        if v is not None and np.array_equal(nv.view(np.uint32), v.view(np.uint32)):
            return v
        v = nv
        alphas = iterate(v, levels, 0.0, 1.0)["alphas"]
    raise AssertionError("adversarial(): the boundary values and the scales they are boundaries of did not meet")


def adversarial(levels=4, seed=125):
    """relu(20011) followed by tiny non-zero values (they belong on the list of non-zeros), negative zeros, negatives under
    lo = 0 (decided at every scale) and, twice each, boundary_triples of the FIRST ADVERSARIAL_SCALES scales the fit
    classifies at - values whose level the fp32 screen cannot settle.

    Why those scales and not the converged one: a value on a boundary of the scale a* makes the update a -> sum b v / sum b b
    jump at a* (by ~1e-5 relative per value), and the fit stops a step of 1e-5 short of its limit, so a tensor whose
    converged scale has values within an ulp of its own boundaries does not exist in general - appending them and fitting
    again cycles.  The scales the kernel classifies AT are what its level arithmetic sees, and the first ones can be met
    exactly: alpha_0 = sum|v| / n is set by one free value at the end of the tensor, and alpha_1, alpha_2 depend smoothly on
    the appended values (they are classified at EARLIER scales there), so rebuilding the triples from the fit of the last
    tensor reaches a tensor that reproduces itself bit for bit; anything else raises.  Pinned in
    tests/test_fp_bracket_ref_cpu.py: at each of those scales the triples of the tensor straddle the boundaries."""
    return _adversarial(levels, seed).copy()


