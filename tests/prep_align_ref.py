"""The numpy restatement of effq_prep_align (the rule of prep.py's --prep_align): fp64 coordinates in the stated order,
fp32 weights and sums on arrays of dtype float32, so that the device can be asked for the same bits."""
import numpy as np


def coordinates(matrix, out_shape):
    """s_a = ((m[a][0] d + m[a][1] h) + m[a][2] w) + m[a][3] in fp64 for every output voxel: three OD x OH x OW arrays."""
    m = np.asarray(matrix, dtype=np.float64).reshape(3, 4)
    d, h, w = (np.arange(n, dtype=np.float64).reshape(s) for n, s in zip(out_shape, ((-1, 1, 1), (1, -1, 1), (1, 1, -1))))
    with np.errstate(all="ignore"):
        return [((m[a, 0] * d + m[a, 1] * h) + m[a, 2] * w) + m[a, 3] for a in range(3)]


def field_of_view(s, shape):
    """-0.5 <= s_a < n_a - 0.5 on all three axes (false for a NaN)."""
    inside = np.ones(s[0].shape, dtype=bool)
    for sa, n in zip(s, shape):
        inside &= (sa >= -0.5) & (sa < float(n) - 0.5)
    return inside


def align(x, matrix, out_shape, nearest=False):
    """(y, inside count) of the D x H x W array `x` (float32, or uint8 with `nearest`) on the grid of `out_shape`."""
    x = np.asarray(x)
    assert x.dtype == (np.uint8 if nearest else np.float32) and x.ndim == 3
    s = coordinates(matrix, out_shape)
    inside = field_of_view(s, x.shape)
    y = np.zeros(tuple(out_shape), dtype=x.dtype)
    at = np.nonzero(inside)
    if nearest:
        idx = [np.minimum(np.floor(sa[at] + 0.5).astype(np.int64), n - 1) for sa, n in zip(s, x.shape)]
        y[at] = x[idx[0], idx[1], idx[2]]
        return y, int(inside.sum())
    i0, i1, l0, l1 = [], [], [], []
    for sa, n in zip(s, x.shape):
        c = np.clip(sa[at], 0.0, float(n - 1))
        fl = np.floor(c)
        lo = fl.astype(np.int64)
        i0.append(lo)
        i1.append(lo + (lo < n - 1))
        l1.append((c - fl).astype(np.float32))
        l0.append(np.float32(1.0) - l1[-1])
    (d0, h0, w0), (d1, h1, w1) = i0, i1
    (ld0, lh0, lw0), (ld1, lh1, lw1) = l0, l1
    with np.errstate(all="ignore"):       # a NaN or an Inf among the eight reaches the output, also at weight 0
        a = ld0 * (lh0 * (lw0 * x[d0, h0, w0] + lw1 * x[d0, h0, w1]) + lh1 * (lw0 * x[d0, h1, w0] + lw1 * x[d0, h1, w1]))
        b = ld1 * (lh0 * (lw0 * x[d1, h0, w0] + lw1 * x[d1, h0, w1]) + lh1 * (lw0 * x[d1, h1, w0] + lw1 * x[d1, h1, w1]))
        v = a + b
    assert v.dtype == np.float32
    y[at] = v
    return y, int(inside.sum())


# ---- grids for the tests ---------------------------------------------------------------------------------------------------
def rotation(axis: int, degrees: float) -> np.ndarray:
    """The 3 x 3 rotation about world axis `axis`."""
    t = np.deg2rad(degrees)
    c, s = np.cos(t), np.sin(t)
    i, j = [k for k in range(3) if k != axis]
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def affine(spacing, origin=(0.0, 0.0, 0.0), rot=None) -> np.ndarray:
    """The 4 x 4 voxel-to-world affine rot diag(spacing) with the translation `origin` (mm)."""
    a = np.eye(4)
    a[:3, :3] = (np.eye(3) if rot is None else rot) @ np.diag(np.asarray(spacing, dtype=np.float64))
    a[:3, 3] = origin
    return a


def oblique_pair():
    """The oblique case of the tests: the source 11 x 13 x 17 of spacing (2, 0.9, 1.1) turned 10 degrees and shifted by
    (-3, 2, 1) mm, the reference 19 x 23 x 37 of spacing (1, 1, 1.5): (A_src, source shape, A_ref, reference shape)."""
    return affine((2.0, 0.9, 1.1), (-3.0, 2.0, 1.0), rotation(2, 10.0)), (11, 13, 17), affine((1.0, 1.0, 1.5)), (19, 23, 37)
