"""The anti-alias filter of `--prep_antialias` restated in numpy fp64 from its definition (include/effq_hip.h,
effq_prep_smooth), not from the kernel: per axis of resampling factor f

    sigma = (f - 1) / 2 if f > 1 else 0,   r = int(4 sigma + 0.5),   g_k = exp(-k^2 / (2 sigma^2)) / sum, k = -r .. r,

the taps rounded to float32 as the device gets them, y[i] = sum_k g_k x[clamp(i + k, 0, n - 1)] along the axis, the
axes one after the other W, H, D, and with keep_zero a voxel that is exactly 0 in the input exactly 0 in the output.
Everything after the taps' rounding is fp64: the GPU tests bound the device's fp32 sums against it."""
import numpy as np

TRUNCATE = 4.0
MAX_RADIUS = 32


def ref_sigma(factor):
    return (float(factor) - 1.0) / 2.0 if factor > 1.0 else 0.0


def ref_radius(sigma):
    return int(TRUNCATE * sigma + 0.5)


def ref_taps(sigma, rounded=True):
    """All 2 r + 1 taps, k = -r .. r, fp64; `rounded`: the values of the float32 taps, not normalised again."""
    r = ref_radius(sigma)
    if r == 0:
        return np.ones(1)
    g = np.array([np.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(-r, r + 1)], dtype=np.float64)
    g = g / g.sum()
    return g.astype(np.float32).astype(np.float64) if rounded else g


def ref_smooth_axis(x, taps, axis):
    """sum_k g_k x[clamp(i + k)] along `axis` of the fp64 array x; taps k = -r .. r."""
    r = (len(taps) - 1) // 2
    n = x.shape[axis]
    i = np.arange(n)
    y = np.zeros(x.shape, dtype=np.float64)
    for k in range(-r, r + 1):
        y += taps[k + r] * np.take(x, np.clip(i + k, 0, n - 1), axis=axis)
    return y


def ref_smooth(x, sigmas, keep_zero=False, rounded=True):
    """x (..., D, H, W) filtered along its last three axes with `sigmas` = (d, h, w), W first; fp64."""
    with np.errstate(invalid="ignore"):
        y = np.asarray(x, dtype=np.float64)
        for axis, sigma in ((-1, sigmas[2]), (-2, sigmas[1]), (-3, sigmas[0])):
            if ref_radius(sigma) > 0:
                y = ref_smooth_axis(y, ref_taps(sigma, rounded), axis)
    return np.where(np.asarray(x) == 0, 0.0, y) if keep_zero else y


def ref_bound(x, sigmas):
    """The device's fp32 result against float32(ref_smooth): per filtered axis an fp32 sum of 2 r + 1 products with
    float32 taps, (2 r + 3) 2^-24 max |x|; the later passes are averages and do not amplify the earlier ones' error."""
    top = float(np.abs(np.asarray(x, dtype=np.float64)[np.isfinite(x)]).max()) if np.isfinite(x).any() else 0.0
    return sum(2 * ref_radius(s) + 3 for s in sigmas if ref_radius(s) > 0) * 2.0 ** -24 * top
