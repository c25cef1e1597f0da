"""The projection + dual update of an ADMM iteration (EfficientQConv.py:108-111, 129-137) restated in numpy, and the inputs
on which the kernels of csrc/project_dual.{h,hip} can go wrong (tests/test_projection_{cpu,gpu}.py).

ref_project does the level arithmetic in fp64 and the rest in fp32, one rounding per step and in the kernels' order: the
library is built with -ffp-contract=off, so numpy's float32 operations give the kernels' bits and every comparison is an
equality.  projection_values returns fp32 inputs on and around every rounding boundary of a scale."""
import ctypes as C

import numpy as np

F32 = np.float32


class ProjNext(C.Structure):
    """effq::ProjNext of csrc/project_dual.h (48 bytes)."""
    _fields_ = [("Bm", C.c_void_p), ("B0", C.c_void_p), ("W0", C.c_void_p), ("nwrow", C.c_int), ("n", C.c_int),
                ("ldb", C.c_int), ("rho", C.c_float), ("eta", C.c_float)]


class ProjFused(C.Structure):
    """effq::ProjFused of csrc/project_dual.h (112 bytes)."""
    _fields_ = [("wstar", C.c_void_p), ("G", C.c_void_p), ("dual", C.c_void_p), ("Gq", C.c_void_p),
                ("err_flag", C.c_void_p), ("d", C.c_double), ("dual_div", C.c_float), ("lm1", C.c_int),
                ("n4", C.c_uint), ("nx", ProjNext)]


# the fp32 screen of csrc/fp_level.h hands a value to the fp64 arithmetic when u lies this close to a rounding boundary
SCREEN_BAND = 0.5 - float(F32(0.4998))
HAND_SCALES = (1e-6, 0.0371234567, 0.73, 1e3)          # 1 / alpha is inexact for each


def ref_levels(v, alpha, levels):
    """Level index of the fp32 values v at scale alpha (fp64): t = v / alpha clamped to [-1, 1], r = rint((t + 1) / d)."""
    d = 2.0 / float(levels - 1)
    with np.errstate(over="ignore"):
        t = np.asarray(v, dtype=np.float64) / float(alpha)
    t = np.minimum(np.maximum(t, -1.0), 1.0)
    return np.rint((t - -1.0) / d), d


def ref_project(v, wstar, dual, alpha, levels, dual_div, nxt=None):
    """(level int64, G f32, dual' f32, Gq int8 or None above 256 levels, Bm f32 or None).

    nxt: dict(B0 (c2, n) f32, W0 (c2 * nwrow) f32, nwrow, n, ldb, rho, eta, fill) - Bm is returned (c2, ldb), its weight
    columns computed and every other element left at `fill`."""
    v, wstar, dual = (np.ascontiguousarray(a, dtype=F32).reshape(-1) for a in (v, wstar, dual))
    r, d = ref_levels(v, alpha, levels)
    b = (r * d + -1.0).astype(F32)
    G = F32(alpha) * b
    du = (wstar - G) + dual
    if F32(dual_div) != F32(1.0):
        du = du / F32(dual_div)
    level = r.astype(np.int64)
    Gq = None
    if levels <= 256:
        q = 2 * level - (levels - 1) if levels <= 128 else level - 128
        assert q.min() >= -128 and q.max() <= 127
        Gq = q.astype(np.int8)
    Bm = None
    if nxt is not None:
        c2, nwrow = nxt["B0"].shape[0], nxt["nwrow"]
        assert v.size == c2 * nwrow and nxt["B0"].shape == (c2, nxt["n"])
        t = nxt["B0"][:, :nwrow].astype(F32) + F32(nxt["eta"]) * nxt["W0"].astype(F32).reshape(c2, nwrow)
        Bm = np.full((c2, nxt["ldb"]), nxt["fill"], dtype=F32)
        Bm[:, :nwrow] = t + F32(nxt["rho"]) * (G - du).reshape(c2, nwrow)
    assert G.dtype == F32 and du.dtype == F32 and (Bm is None or Bm.dtype == F32)
    return level, G, du, Gq, Bm


def ulp_shift(x, k):
    """The fp32 values k units in the last place above (k < 0: below) x; -0.0 and +0.0 count as one value."""
    i = np.ascontiguousarray(x, dtype=F32).view(np.int32).astype(np.int64)
    m = np.where(i >= 0, i, -(i & 0x7FFFFFFF)) + int(k)
    back = np.where(m >= 0, m, (-m) | 0x80000000).astype(np.uint32)
    return back.view(F32)


def special_values(alpha, levels, seed):
    """fp32 values at which the level of the scale alpha is decided by the last bits: every rounding boundary
    alpha ((j + 0.5) d - 1) with its neighbours at +-1, +-2 and +-4 ulp and >= 600 values spread over +-3e-4 levels around
    the boundaries (both sides of the screen's band of 2e-4), every level centre, +-alpha with the same neighbours,
    +-10 alpha, +-0.0, a subnormal and +-inf."""
    rng = np.random.default_rng(seed)
    d = 2.0 / float(levels - 1)
    j = np.arange(levels - 1, dtype=np.float64)
    bnd = (float(alpha) * ((j + 0.5) * d - 1.0)).astype(F32)
    out = [ulp_shift(bnd, k) for k in (0, 1, -1, 2, -2, 4, -4)]
    per = -(-600 // (levels - 1))
    jj = np.repeat(j, per)
    off = rng.uniform(-3e-4, 3e-4, jj.size)
    out.append((float(alpha) * ((jj + 0.5 + off) * d - 1.0)).astype(F32))
    out.append((float(alpha) * (np.arange(levels, dtype=np.float64) * d - 1.0)).astype(F32))
    ends = np.array([alpha, -alpha], dtype=np.float64).astype(F32)
    out += [ulp_shift(ends, k) for k in (0, 1, -1, 2, -2, 4, -4)]
    out.append(np.array([10.0 * alpha, -10.0 * alpha], dtype=np.float64).astype(F32))
    out.append(np.array([0.0, -0.0, 1e-40, np.inf, -np.inf], dtype=F32))
    return np.concatenate(out)


def projection_values(alpha, levels, n, seed):
    """n fp32 inputs of the projection at scale alpha, deterministic by seed: special_values and a normal fill of spread
    0.6 alpha, shuffled; where n is smaller than the number of special values, a random n of them."""
    rng = np.random.default_rng(seed + 7919)
    sp = special_values(alpha, levels, seed)
    if n > sp.size:
        sp = np.concatenate([sp, (0.6 * float(alpha) * rng.standard_normal(n - sp.size)).astype(F32)])
    return np.ascontiguousarray(sp[rng.permutation(sp.size)[:n]])


def screen_fallbacks(v, alpha, levels):
    """How many of the values v the fp32 screen of csrc/fp_level.h hands to the fp64 arithmetic (emulated: the product is
    exact in fp64, so at most a double rounding separates this u from the kernel's fused multiply-add)."""
    d = 2.0 / float(levels - 1)
    rd = 1.0 / d
    c1, c0, lmax = F32((1.0 / float(alpha)) * rd), F32(1.0 * rd), F32(np.rint(2.0 * rd))
    with np.errstate(over="ignore", invalid="ignore"):
        u = (np.asarray(v, dtype=np.float64) * float(c1) + float(c0)).astype(F32)
    u = np.minimum(np.maximum(u, F32(0.0)), lmax)
    return int(np.count_nonzero(~(np.abs(u - np.rint(u)) < F32(0.4998))))


def host_state(alpha, iters=1, done=1):
    """effq_fp_state (include/effq_hip.h) as the 5 doubles hip_ops.new_fp_state allocates."""
    st = np.zeros(5, dtype=np.float64)
    st[0], st[1] = alpha, alpha
    st[4:5].view(np.int32)[:] = (iters, done)
    return st
