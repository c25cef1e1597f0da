"""Bit-exact host models of the exact-integer conv kernels and the probe targets that turn their two loss sums into a
check of every single output.

The loss-only conv kernels return sum (out - y)^2 and nothing else.  Against a random y that sum cannot see one wrong, omitted
or doubled output.  The integer epilogues, though, can be restated bit for bit in numpy float32 (the library is built with
-ffp-contract=off, nothing is fused):

    scale = f32( f64(f32 a_act) * f64(f32 a_w) * (1.0 / ((La - 1)(Lw - 1))) )      products in that order, inv_levels a double
    out   = f32( f32( f32(num) * scale ) + bias )                                  bias = +0.0f without one

with num the exact int32 accumulator (conv3d_i8.hip: epilogue_scale, epilogue_cells / _even / _masked; conv3d_i8s.hip: the
numerator of its header comment).  With y equal to that model both sums are 0.0 exactly.  With y moved off the model by
exactly +-0.5 on a probe set P - the sign chosen per output so that f32(o - y) is +-0.5 exactly - every squared error is 0.25 or
0, every fp32 and fp64 partial sum is exact in any order, and the sums must be 0.25 |P| and 0.25 sum_P att exactly (att in
{0.25, 1, 3.5}).  Probe sets: nothing, everything, and one set per bit of each output coordinate; an output that is left out
or counted twice fails exactly the planes whose bit is set in its coordinates, which explain() spells out.

Imports without a device."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

AXES = ("n", "od", "oh", "ow", "c")
HALF = np.float32(0.5)


def _triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(int(i) for i in v)


# ------------------------------------------------------------------ the epilogue, bit for bit
def epilogue_scale(a_act, a_w, la, lw):
    """epilogue_scale (conv3d_i8.hip) / line 131 of conv3d_i8s.hip: one rounding of a product of three doubles."""
    inv_levels = 1.0 / (float(la - 1) * float(lw - 1))
    return np.float32(float(np.float32(a_act)) * float(np.float32(a_w)) * inv_levels)


def int_conv(x_ndhwc, w, stride=1, pad=0):
    """conv3d of integer tensors (x [N][D][H][W][C1], w [C2][C1][kd][kh][kw]) as int64 [N][OD][OH][OW][C2].  Computed in fp64:
    exact while every sum stays below 2^53, here 2^31."""
    out = F.conv3d(x_ndhwc.permute(0, 4, 1, 2, 3).double(), w.double(), None, stride, pad)
    out = out.permute(0, 2, 3, 4, 1).contiguous()
    assert float(out.abs().max()) < 2.0 ** 31, "the numerator leaves int32"
    assert bool((out == out.round()).all())
    return out.numpy().astype(np.int64)


def scale_bias(num, scale, bias):
    """f32( f32( f32(num) * scale ) + bias ): three roundings in numpy float32, the conversion included."""
    assert np.abs(num).max() < 2 ** 31
    t = num.astype(np.int32).astype(np.float32) * np.float32(scale)
    b = np.zeros(num.shape[-1], np.float32) if bias is None else np.asarray(bias, dtype=np.float32)
    out = t + b
    assert out.dtype == np.float32
    return out


def i8_model(xidx, gq, bias, a_act, a_w, la, lw, pad):
    """The outputs of conv3d_calib_step_i8 / conv3d_quant_forward_i8, float32 [N][OD][OH][OW][C2], and their numerators.
    xidx: uint8 level ids, NDHWC; gq: int8 numerators 2 * level - (Lw - 1), [C2][C1][3][3][3]; bias: float32 [C2] or None."""
    num = int_conv(xidx, gq, 1, pad)
    b = None if bias is None else bias.numpy()
    return scale_bias(num, epilogue_scale(a_act, a_w, la, lw), b), num


def i8s_operand(m, lw):
    """The int8 weight operand of numerator m = 2 * level - (Lw - 1): m itself, or level - 128 = (m - 1) / 2 at 256 levels."""
    return (m - 1) // 2 if lw > 128 else m


def i8s_numerator(gop, lw):
    return 2 * gop + 1 if lw > 128 else gop


def i8s_parts(xidx, gop, la, lw, stride, pad):
    """The integers of conv3d_i8s.hip's header: acc over all taps with the re-centred operands (padding = -128 when La > 128),
    Ksum per output channel, Su per output voxel, and the constants aoff and wmul."""
    aoff = 128 if la > 128 else 0
    wmul = 2 if lw > 128 else 1
    pd, ph, pw = _triple(pad)
    x = xidx.permute(0, 4, 1, 2, 3).double()
    a_op = F.pad(x - aoff, (pw, pw, ph, ph, pd, pd), value=float(-aoff))
    assert float(a_op.min()) >= -128 and float(a_op.max()) <= 127
    acc = F.conv3d(a_op, gop.double(), None, stride, 0).permute(0, 2, 3, 4, 1).contiguous().numpy().astype(np.int64)
    ksum = gop.double().sum(dim=(1, 2, 3, 4)).numpy().astype(np.int64)
    ones = torch.ones(1, *gop.shape[1:], dtype=torch.float64)
    su = F.conv3d(x, ones, None, stride, pad).permute(0, 2, 3, 4, 1).contiguous().numpy().astype(np.int64)
    return dict(acc=acc, ksum=ksum, su=su, aoff=aoff, wmul=wmul)


def i8s_model(xidx, gop, bias, a_act, a_w, la, lw, stride, pad):
    """The outputs of conv3d_calib_step_i8s and their numerators wmul * (acc + aoff * Ksum) + (Lw > 128 ? Su : 0), every
    intermediate inside int32 as in the kernel.  gop: the int8 weight operands (i8s_operand), [C2][C1][kd][kh][kw]."""
    p = i8s_parts(xidx, gop, la, lw, stride, pad)
    inner = p["acc"] + p["aoff"] * p["ksum"]
    num = p["wmul"] * inner + (p["su"] if lw > 128 else 0)
    for v in (p["acc"], inner, num):
        assert np.abs(v).max() < 2 ** 31
    b = None if bias is None else bias.numpy()
    return scale_bias(num, epilogue_scale(a_act, a_w, la, lw), b), num


# ------------------------------------------------------------------ the probes
def probe_targets(o):
    """For every output the target half a unit away from it: y with f32(o - y) == +0.5 exactly where o - 0.5 allows it, else
    the one with f32(o - y) == -0.5.  One of the two signs must be exact at every output: no output may be left out of a
    probe set.  Returns (targets, share of outputs that needed the second sign)."""
    assert o.dtype == np.float32
    y_lo, y_hi = o - HALF, o + HALF
    ok_lo, ok_hi = (o - y_lo) == HALF, (o - y_hi) == -HALF
    bad = ~(ok_lo | ok_hi)
    assert not bad.any(), f"{int(bad.sum())} outputs take neither sign exactly, e.g. {o[bad][:4]}"
    return np.where(ok_lo, y_lo, y_hi), float((~ok_lo).mean())


def probe_sets(shape):
    """(name, boolean mask broadcastable to `shape`) of the empty set, the full set and, per axis of [N][OD][OH][OW][C2] and
    per bit of its coordinate, the outputs whose coordinate has that bit set."""
    yield "zero", np.zeros((1,) * 5, bool)
    yield "full", np.ones((1,) * 5, bool)
    for ax, (name, n) in enumerate(zip(AXES, shape)):
        for bit in range(max(n - 1, 0).bit_length()):
            view = [1] * 5
            view[ax] = n
            yield f"{name}.{bit}", (((np.arange(n) >> bit) & 1) == 1).reshape(view)


def probe(o, targets, mask, att=None):
    """y = the half-unit target on the probe set, the model elsewhere; the exact sums 0.25 |P| and 0.25 sum_P att (the
    unweighted one again without att).  att: float [N][OD][OH][OW] with dyadic values."""
    m = np.broadcast_to(mask, o.shape)
    y = np.where(m, targets, o)
    s0 = 0.25 * float(m.sum())
    s1 = s0 if att is None else 0.25 * float((np.asarray(att, dtype=np.float64)[..., None] * m).sum())
    return y, s0, s1


def brute_force_sums(o, y, att=None):
    """What a kernel computes from outputs o: d = f32(o - y), f32(d * d), f32(att * d^2), summed (here in fp64)."""
    d = o - y
    sq = d * d
    assert sq.dtype == np.float32
    s0 = float(sq.astype(np.float64).sum())
    if att is None:
        return s0, s0
    w = np.asarray(att, dtype=np.float32)[..., None] * sq
    assert w.dtype == np.float32
    return s0, float(w.astype(np.float64).sum())


def explain(fails, shape):
    """The assertion message for a list of failed probes (name, got [s0, s1], want [s0, s1])."""
    lines = [f"{name}: got {got}, want {want}, off by {[g - w for g, w in zip(got, want)]}" for name, got, want in fails]
    failed = {name for name, _, _ in fails}
    if "zero" in failed:
        lines.append("the zero-residual probe fails: some output differs from the model (or the model is wrong)")
    coord = {}
    for name, n in zip(AXES, shape):
        bits = [b for b in range(max(n - 1, 0).bit_length()) if f"{name}.{b}" in failed]
        coord[name] = sum(1 << b for b in bits)
    lines.append(f"planes that fail have these bits set - a single output left out or doubled sits at {coord} of {tuple(shape)}")
    return "\n".join(lines)


def run_family(launch, o, att=None, only=None):
    """launch(y float32 ndarray) -> [s0, s1] for every probe set (or those named in `only`); exact equality of both sums.
    Returns the number of probes."""
    targets, _ = probe_targets(o)
    fails, count = [], 0
    for name, mask in probe_sets(o.shape):
        if only is not None and name not in only:
            continue
        y, s0, s1 = probe(o, targets, mask, att)
        got = [float(v) for v in launch(y)]
        count += 1
        if got != [s0, s1]:
            fails.append((name, got, [s0, s1]))
    assert not fails, explain(fails, o.shape)
    return count


# ------------------------------------------------------------------ host problems of the GPU cases (shared with the CPU test)
A_ACT = np.float32(0.8123)
PATTERNS = ("pos", "neg", "checker", "odd")


def _a_w(k):
    return np.float32(3.0 / k ** 0.5)                                # as _i8_host_problem: random outputs of order one


def saturated_tiled(c1, c2, sp, la, lw, pattern):
    """Operands at the extremes.  pos / neg: every id at La - 1, every numerator at +(Lw - 1) / -(Lw - 1).  checker: ids La - 1
    where channel + d + h + w is even and 0 elsewhere, numerators (Lw - 1) (-1)^(c2 + c1 + tap): under one output every
    non-zero product has the same sign, so the numerators stay large and alternate in sign from output to output.  odd: as pos
    with the ids of channel 0 at La - 2.  (In the first three every numerator is a multiple of C1 / 2 with an odd part below
    2^24: f32(num) is exact however large num is.  With one channel a level lower the large numerators are odd.)"""
    n = 2
    if pattern == "checker":
        grid = np.indices((n, *sp, c1))
        xidx = torch.from_numpy((((grid[1] + grid[2] + grid[3] + grid[4]) % 2 == 0) * (la - 1)).astype(np.uint8))
        g = np.indices((c2, c1, 27))
        gq = torch.from_numpy((np.where((g[0] + g[1] + g[2]) % 2 == 0, lw - 1, -(lw - 1))).astype(np.int64))
        gq = gq.reshape(c2, c1, 3, 3, 3)
    else:
        xidx = torch.full((n, *sp, c1), la - 1, dtype=torch.uint8)
        gq = torch.full((c2, c1, 3, 3, 3), -(lw - 1) if pattern == "neg" else (lw - 1), dtype=torch.int64)
        if pattern == "odd":
            xidx[..., 0] = la - 2
    return xidx, gq


@functools.lru_cache(maxsize=None)
def saturated_i8_problem(c1, c2, out, pad, la, lw, with_bias, pattern):
    """A problem in the form of test_conv_geometry_gpu._i8_host_problem with saturated operands; y is the model itself."""
    sp = tuple(o + 2 - 2 * p for o, p in zip(out, _triple(pad)))
    gen = torch.Generator().manual_seed(911 + c1 + 3 * c2 + sum(out))
    xidx, gq = saturated_tiled(c1, c2, sp, la, lw, pattern)
    gq = gq.to(torch.int8)
    b = torch.randn(c2, generator=gen) * 0.1 if with_bias else None
    att = torch.tensor([0.25, 1.0, 3.5])[torch.randint(0, 3, (2, *out), generator=gen)]
    a_w = _a_w(27 * c1)
    o, num = i8_model(xidx, gq, b, A_ACT, a_w, la, lw, pad)
    return dict(sp=sp, xidx=xidx, gq=gq, a_act=A_ACT, a_w=a_w, b=b, y=torch.from_numpy(o), att=att, o=o, num=num)


# short-K cases beyond test_conv_geometry_gpu.I8S: K = 256, the longest i8s_plan takes (16 channels x 2 x 2 x 4 taps, NJ = 8)
I8S_EXTRA = {
    "16to32_k224_K256_256_256": (16, 32, (2, 2, 4), 1, (1, 0, 2), 256, 256, (6, 7, 9), (8, 1, 128, 2)),
}
I8S_SATURATED = ("4to32_p2_recentred_256_256", "16to32_k224_K256_256_256")


def i8s_case(case):
    from tests.test_conv_geometry_gpu import I8S
    return I8S[case] if case in I8S else I8S_EXTRA[case]


@functools.lru_cache(maxsize=None)
def i8s_problem(case, pattern=None):
    """Random (pattern None) or saturated operands of a short-K case, N = 2, and the model."""
    c1, c2, k, s, p, la, lw, sp, _ = i8s_case(case)
    kk = _triple(k)
    n = 2
    gen = torch.Generator().manual_seed(4242 + c1 + 7 * c2 + la + 3 * lw + sum(kk) + sum(sp))
    if pattern is None:
        xidx = torch.randint(0, la, (n, *sp, c1), generator=gen, dtype=torch.uint8)
        m = 2 * torch.randint(0, lw, (c2, c1, *kk), generator=gen) - (lw - 1)
    elif pattern == "checker":
        grid = np.indices((n, *sp, c1))
        xidx = torch.from_numpy((((grid[1] + grid[2] + grid[3] + grid[4]) % 2 == 0) * (la - 1)).astype(np.uint8))
        g = np.indices((c2, c1, *kk))
        m = torch.from_numpy(np.where((g[0] + g[1] + g[2] + g[3] + g[4]) % 2 == 0, lw - 1, -(lw - 1)).astype(np.int64))
    else:
        xidx = torch.full((n, *sp, c1), la - 1, dtype=torch.uint8)
        m = torch.full((c2, c1, *kk), -(lw - 1) if pattern == "neg" else (lw - 1), dtype=torch.int64)
        if pattern == "odd":
            xidx[..., 0] = la - 2
    gop = i8s_operand(m, lw).to(torch.int8)
    assert torch.equal(i8s_numerator(gop.long(), lw), m.long())
    b = torch.randn(c2, generator=gen) * 0.1
    a_w = _a_w(c1 * math.prod(kk))
    o, num = i8s_model(xidx, gop, b, A_ACT, a_w, la, lw, s, p)
    return dict(xidx=xidx, gop=gop, m=m, b=b, a_act=A_ACT, a_w=a_w, o=o, num=num)


def bump_one_numerator(gq, c2, c1, tap, lw):
    """gq with the numerator at (c2, c1, tap) moved by one level (2), inwards at the ends of the range; returns (new, step)."""
    g = gq.clone()
    flat = g.view(g.shape[0], g.shape[1], -1)
    step = -2 if int(flat[c2, c1, tap]) + 2 > lw - 1 else 2
    flat[c2, c1, tap] += step
    return g, step
