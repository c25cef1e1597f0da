"""The numpy restatement of effq_seg_probs_source (`predict --save_prob / --save_unc`), shared by test_seg_prob_cpu and
test_seg_prob_gpu.

Two steps.  ref_logits_source is the fp32 restatement of the interpolation: the per-axis map and inside rule of
tests.test_predict_cpu.ref_axis_source (fp64), the weights l1 = float32(q - i0), l0 = 1.0f - l1, and the eight corners
combined in fp32 in the corner order of ref_labels_source, one rounding per operation - what the kernels compute, bit
for bit.  ref_probs_source takes those fp32 values and computes the probabilities and the uncertainty in fp64 with the
definitions of DESIGN section 20, and returns the exact real values 255 p and 255 u the stored bytes are rounded from.

E_PROB and E_UNC are the fp32 error of the device formulation in levels (derived from the
operation count with expf and logf within 3 ulp and the division within 2.5 ulp): every stored byte q must satisfy
|q - 255 x| <= 0.5 + E, and a NaN x is stored as 0."""
import numpy as np

from tests.test_predict_cpu import ref_axis_source

EPS = 2.0 ** -23
E_PROB = 255.0 * 16.0 * EPS          # 4.9e-4 of a level
E_UNC = 255.0 * 32.0 * EPS           # 9.7e-4 of a level


def ref_logits_source(logits, pmin, grid, factors, source_shape):
    """(v, inside): the C x source fp32 logits interpolated as k_seg_labels_source interpolates them (also where the
    voxel is outside, from the clamped coordinates), and the inside mask."""
    x = np.ascontiguousarray(logits, dtype=np.float32)
    box = x.shape[1:]
    f = (1.0, 1.0, 1.0) if factors is None else factors
    axes = [ref_axis_source(n, fa, G, lo, g) for n, fa, G, lo, g in zip(source_shape, f, grid, pmin, box)]
    (md, d0, d1, _), (mh, h0, h1, _), (mw, w0, w1, _) = axes
    l1 = [a[3].astype(np.float32) for a in axes]
    l0 = [np.float32(1.0) - l for l in l1]
    inside = md[:, None, None] & mh[None, :, None] & mw[None, None, :]
    d_0, d_1 = l0[0][:, None, None], l1[0][:, None, None]
    h_0, h_1 = l0[1][None, :, None], l1[1][None, :, None]
    w_0, w_1 = l0[2][None, None, :], l1[2][None, None, :]
    at = lambda d, h, w: x[:, d[:, None, None], h[None, :, None], w[None, None, :]]
    with np.errstate(invalid="ignore", over="ignore"):
        a = d_0 * (h_0 * (w_0 * at(d0, h0, w0) + w_1 * at(d0, h0, w1)) + h_1 * (w_0 * at(d0, h1, w0) + w_1 * at(d0, h1, w1)))
        b = d_1 * (h_0 * (w_0 * at(d1, h0, w0) + w_1 * at(d1, h0, w1)) + h_1 * (w_0 * at(d1, h1, w0) + w_1 * at(d1, h1, w1)))
        v = a + b
    assert v.dtype == np.float32
    return v, inside


def probs_of(v, mode):
    """(p, u) in fp64 of C x ... fp32 logits: the definitions of DESIGN section 20, limits for infinite logits, NaN for
    NaN."""
    v = np.asarray(v, dtype=np.float64)
    C = v.shape[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if mode == "argmax":
            m = np.max(v, 0)                                     # a NaN channel makes everything NaN either way
            d = np.where(v == m, 0.0, v - m)
            e = np.exp(d)
            S = e.sum(0)
            p = e / S
            if C == 1:
                return p, np.where(np.isnan(p[0]), np.nan, 0.0)
            u = (np.log(S) - np.where(e > 0, p * d, 0.0).sum(0)) / np.log(float(C))
            return p, np.where(np.isnan(S), np.nan, u)
        assert mode == "sigmoid"
        p = 1.0 / (1.0 + np.exp(-v))
        a = np.abs(v)
        t = np.exp(-a)
        h = np.where(t > 0, (np.log1p(t) + a * t / (1.0 + t)) / np.log(2.0), 0.0)
        h = np.where(np.isnan(v), np.nan, h)
        return p, np.max(h, 0)                                   # np.max: a NaN channel makes u NaN


def ref_probs_source(logits, pmin, grid, factors, source_shape, mode, interp=None):
    """(P, U, inside, v): the exact real values 255 p (C x source) and 255 u (source) in fp64 - NaN where the device
    stores 0 for a NaN - with the values of outside voxels (sigmoid: 0; argmax: channel 0 = 255, the others 0; u = 0),
    the inside mask and the interpolated fp32 logits.  `interp`: (v, inside) of an earlier ref_logits_source of the same
    arguments, to share it between the modes."""
    v, inside = interp if interp is not None else ref_logits_source(logits, pmin, grid, factors, source_shape)
    p, u = probs_of(v, mode)
    P, U = 255.0 * p, 255.0 * u
    P[:, ~inside] = 0.0
    if mode == "argmax":
        P[0, ~inside] = 255.0
    U[~inside] = 0.0
    return P, U, inside, v


def stored(x255):
    """The byte of an exact value 255 x: nearest, half to even, NaN -> 0."""
    x = np.asarray(x255, dtype=np.float64)
    return np.where(np.isnan(x), 0.0, np.rint(np.clip(x, 0.0, 255.0))).astype(np.uint8)


def check_stored(q, x255, E, tag=""):
    """Every byte within 0.5 + E of the exact value; a NaN value stored as 0.  Returns the largest |q - 255 x|."""
    q = np.asarray(q).astype(np.float64)
    x = np.asarray(x255, dtype=np.float64)
    nan = np.isnan(x)
    assert not q[nan].any(), f"{tag}: a NaN value is stored as 0"
    err = np.abs(q - x)[~nan]
    worst = float(err.max()) if err.size else 0.0
    assert worst <= 0.5 + E, f"{tag}: |q - 255 x| = {worst!r} > 0.5 + {E:.3g}"
    return worst
