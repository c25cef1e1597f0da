"""The numpy restatement of the percentile window of prep.py (--prep_window pLO,pHI; the rule at prep.PercentileWindow)
that the tests of effq_prep_quantiles and effq_prep_mask_window share.  Nothing here imports the package."""
import math

import numpy as np

U24 = 2.0 ** -24


def ref_mask(x, mask):
    return np.ones(x.shape, bool) if mask == "all" else x != 0


def ref_sorted(x, mask):
    """The voxels of one modality's mask in the rule's order: ascending, -0.0 as +0.0, every NaN after +Inf."""
    v = np.asarray(x, dtype=np.float32).reshape(-1)
    v = v[ref_mask(v, mask)]
    v = np.where(v == 0, np.float32(0.0), v)        # -0.0 counts as +0.0
    return np.sort(v)                               # numpy sorts every NaN last


def ref_rank(n, q):
    """(h, k) of the rule: h = (n - 1) q / 100 in fp64 with the product first, k = floor(h)."""
    h = float(n - 1) * float(q) / 100.0
    return h, int(math.floor(h))


def ref_stats(x, qs, mask):
    """(n, stats float32[len(qs), 2]) of one modality: sorted[k] and sorted[min(k + 1, n - 1)]; NaN when n = 0."""
    s = ref_sorted(x, mask)
    n = len(s)
    out = np.full((len(qs), 2), np.nan, np.float32)
    for r, q in enumerate(qs):
        if n:
            _, k = ref_rank(n, q)
            out[r] = s[k], s[min(k + 1, n - 1)]
    return n, out


def ref_value(n, q, a, b):
    """The bound of the rule from the two order statistics: the float32 nearest a + (h - k) (b - a), a when a == b."""
    h, k = ref_rank(n, q)
    a, b = np.float64(a), np.float64(b)
    with np.errstate(all="ignore"):
        return np.float32(a if a == b else a + (h - k) * (b - a))


def ref_percentile(x, q, mask):
    n, st = ref_stats(x, [q], mask)
    return ref_value(n, q, st[0, 0], st[0, 1])


def ref_window_mask(x, lo, hi, mask):
    """x clipped to [lo, hi] inside the mask, left alone outside it; a NaN stays."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(ref_mask(x, mask), np.clip(x, np.float32(lo), np.float32(hi)), x)


def same_bits(a, b):
    """Equal bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


def percentile_bound(x, mask):
    """|bound - numpy.percentile(fp64)| allowed: 2^-24 M + 2^-50 n (max - min), M the largest magnitude in the mask: the
    one float32 rounding, and the two roundings of h times the steepest slope of the piecewise-linear function."""
    v = np.asarray(x, np.float64).reshape(-1)
    v = v[ref_mask(v, mask)]
    return U24 * float(np.abs(v).max()) + 2.0 ** -50 * len(v) * float(v.max() - v.min())
