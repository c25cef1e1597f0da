"""The rule of efficientq_amd/denoise.py restated in plain fp64 numpy: the pseudo-residuals, the noise level and the
non-local means filter, displacement by displacement with clamped index arrays."""
import itertools
import math

import numpy as np

H2 = 1.0
MAD_SCALE = 1.4826 * math.sqrt(6.0 / 7.0)


def omega(v, mask="nonzero"):
    return np.isfinite(v) & ((v != 0) if mask == "nonzero" else True)


def residual(v, mask="nonzero"):
    """float32 r: |v - the mean of the six face neighbours| where all seven are inside and in Omega, +0 elsewhere."""
    v = np.asarray(v, dtype=np.float32)
    r = np.zeros(v.shape, dtype=np.float32)
    if min(v.shape) < 3:
        return r
    om, x = omega(v, mask), v.astype(np.float64)
    c = (slice(1, -1),) * 3
    ok, s = om[c].copy(), 0.0
    for axis in range(3):                               # d-, d+, h-, h+, w-, w+: the order of the sum
        for lo in (slice(0, -2), slice(2, None)):
            at = tuple(lo if a == axis else slice(1, -1) for a in range(3))
            ok &= om[at]
            s = s + x[at]
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs((x[c] - s / 6.0).astype(np.float32))
    r[c] = np.where(ok, e, np.float32(0))
    return r


def sigma_of(r):
    """(sigma, n): MAD_SCALE times the median of the non-zero residuals, the median rounded to float32 as the device's
    percentile is."""
    s = np.sort(r[r != 0].astype(np.float64))
    n = s.size
    if n == 0:
        return math.nan, 0
    h, k = (n - 1) * 50.0 / 100.0, (n - 1) // 2
    a, b = s[k], s[min(k + 1, n - 1)]
    return MAD_SCALE * float(np.float32(a if a == b else a + (h - k) * (b - a))), n


def nlm(v, mask, radius, sigma):
    """(y float64, spread, sumsq, count): the filter; y equals v outside Omega.  spread is max - min of the finite v in
    every voxel's search window, the scale of the device's error bound."""
    v32 = np.asarray(v, dtype=np.float32)
    x, om, dims = v32.astype(np.float64), omega(v32, mask), v32.shape
    grid = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    clamp = lambda idx: tuple(np.clip(i, 0, n - 1) for i, n in zip(idx, dims))
    num, den, wmax = np.zeros(dims), np.zeros(dims), np.zeros(dims)
    top, bot = np.where(np.isfinite(x), x, -np.inf), np.where(np.isfinite(x), x, np.inf)
    hi, lo = np.full(dims, -np.inf), np.full(dims, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in itertools.product(range(-radius, radius + 1), repeat=3):
            j = [g + s for g, s in zip(grid, t)]
            inside = np.all([(a >= 0) & (a < n) for a, n in zip(j, dims)], axis=0)
            jc = clamp(j)
            hi, lo = np.maximum(hi, np.where(inside, top[jc], -np.inf)), np.minimum(lo, np.where(inside, bot[jc], np.inf))
            if t == (0, 0, 0):
                continue
            d2 = sum((x[clamp([g + o for g, o in zip(grid, s)])] - x[clamp([a + o for a, o in zip(j, s)])]) ** 2
                     for s in itertools.product((-1, 0, 1), repeat=3)) / 27.0
            w = np.exp(-np.maximum(d2 - 2.0 * sigma ** 2, 0.0) / (H2 * sigma ** 2))
            w = np.where(inside & om[jc] & np.isfinite(d2), w, 0.0)
            num += w * np.where(w > 0, x[jc], 0.0)
            den += w
            wmax = np.maximum(wmax, w)
        wmax = np.where(wmax > 0, wmax, 1.0)
        y = np.where(om, (num + wmax * np.where(om, x, 0.0)) / (den + wmax), x)
        spread = np.where(om, hi - lo, 0.0)
    return y, spread, float(((y[om] - x[om]) ** 2).sum()), int(om.sum())
