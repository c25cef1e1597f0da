"""An fp64 numpy restatement of the rule of `--prep_interp cubic` (the comment at prep.CUBIC_POLE), written from the rule
and not from the kernel: the B-spline prefilter with the whole-sample mirror, the evaluation at the coordinates of the
trilinear path, the zero rule of `--prep_mask nonzero`, and the window applied once more."""
import math

import numpy as np

POLE = math.sqrt(3.0) - 2.0
GAIN = 6.0
U24, TINY = 2.0 ** -24, 2.0 ** -149


def ref_prefilter_axis(x, axis):
    """The coefficients along one axis: (c[k-1] + 4 c[k] + c[k+1]) / 6 = x[k], c[-1] = c[1], c[n] = c[n-2]."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    n = x.shape[0]
    if n == 1:
        return np.moveaxis(x.copy(), 0, axis)
    z = POLE
    k = np.arange(2 * n - 2)
    mirrored = np.where(k < n, k, 2 * n - 2 - k)
    s = np.tensordot(np.power(z, k.astype(np.float64)), x[mirrored], axes=(0, 0))      # one whole period, nothing cut
    cp = np.empty_like(x)
    cp[0] = GAIN * s / (1.0 - z ** (2 * n - 2))
    for i in range(1, n):
        cp[i] = GAIN * x[i] + z * cp[i - 1]
    c = np.empty_like(x)
    c[n - 1] = z / (z * z - 1.0) * (cp[n - 1] + z * cp[n - 2])
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - cp[i])
    return np.moveaxis(c, 0, axis)


def ref_prefilter(x):
    """All three trailing axes, D then H then W."""
    c = np.asarray(x, dtype=np.float64)
    for axis in (-3, -2, -1):
        c = ref_prefilter_axis(c, axis)
    return c


def ref_coords(out, factor, n):
    """s = (o + 0.5) f - 0.5 clamped to [0, n - 1], for o = 0 .. out - 1."""
    s = (np.arange(out, dtype=np.float64) + 0.5) * float(factor) - 0.5
    return np.clip(s, 0.0, float(n - 1))


def ref_axis(out, factor, n):
    """(idx (out, 4), weights (out, 4), i0 (out), i1 (out)): the four mirrored coefficient indices and their weights, and
    the two indices of the trilinear footprint (i1 = i0 where the second does not count)."""
    s = ref_coords(out, factor, n)
    i0 = np.floor(s).astype(np.int64)
    t = s - i0
    i1 = np.where((t > 0) & (i0 < n - 1), i0 + 1, i0)
    if n == 1:
        return np.zeros((out, 4), np.int64), np.tile([0.0, 1.0, 0.0, 0.0], (out, 1)), i0, i1
    idx = i0[:, None] + np.arange(-1, 3)[None, :]
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx >= n, 2 * n - 2 - idx, idx)
    w = np.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6,
                  t ** 3 / 6], axis=1)
    outside = (idx < 0) | (idx >= n)            # i0 + 2 = n + 1 at s = n - 1: mirrored once it is still outside
    assert np.all(w[outside] == 0)
    return np.clip(idx, 0, n - 1), w, i0, i1


def ref_resample_cubic(x, factors, out_shape, zero_keep=False):
    """x (..., D, H, W) -> fp64 (..., OD, OH, OW): prefilter, then the 4 x 4 x 4 evaluation, w innermost, then h, then d;
    with zero_keep a voxel whose trilinear footprint in x is all exactly 0 is 0.  Not rounded to float32."""
    x = np.asarray(x)
    c = ref_prefilter(x)
    zero = x == 0
    for axis, f, o in ((-1, factors[2], out_shape[2]), (-2, factors[1], out_shape[1]), (-3, factors[0], out_shape[0])):
        n = c.shape[axis]
        idx, w, i0, i1 = ref_axis(o, f, n)
        c = np.moveaxis(c, axis, -1)
        acc = w[:, 0] * c[..., idx[:, 0]]
        for j in range(1, 4):
            acc = acc + w[:, j] * c[..., idx[:, j]]
        c = np.moveaxis(acc, -1, axis)
        zero = np.moveaxis(zero, axis, -1)
        zero = np.moveaxis(zero[..., i0] & zero[..., i1], -1, axis)
    return np.where(zero, 0.0, c) if zero_keep else c


def ref_footprint_zero(x, factors, out_shape):
    """The output voxels the zero rule names: every source voxel of the trilinear footprint is exactly 0."""
    zero = np.asarray(x) == 0
    for axis, f, o in ((-1, factors[2], out_shape[2]), (-2, factors[1], out_shape[1]), (-3, factors[0], out_shape[0])):
        _, _, i0, i1 = ref_axis(o, f, zero.shape[axis])
        zero = np.moveaxis(zero, axis, -1)
        zero = np.moveaxis(zero[..., i0] & zero[..., i1], -1, axis)
    return zero


def ref_window(y, lo, hi):
    """The window applied once more after the resampling (numpy.clip)."""
    return np.clip(y, lo, hi)


def ref_tolerance(ref, xmax):
    """|got - ref| for the device's float32 `got`: one rounding to float32 (2^-24 |ref| + 2^-149) plus an fp64 allowance of
    1e-11 max |x| for the order of the sums."""
    return U24 * np.abs(ref) + TINY + 1e-11 * float(xmax)
