"""The projection + dual update that ends every ADMM iteration (EfficientQConv.py:108-111, 129-137), in each of its three
tensor-scale implementations, against the fp64 restatement of tests/projection_ref.py (-m gpu):

  k_project_dual       one element per thread, level from the fp64 arithmetic (misaligned operands, n % 4 != 0, rows % 4 != 0)
  k_project_dual4      16-byte accesses, level from the fp32 screen of csrc/fp_level.h
  proj_fused_epilogue  the same four-wide code as the epilogue of k_fp_small (effq_fixed_point_small_fused)

Levels, G, the new dual, the int8 numerators Gq and the right-hand side Bm of the next prox solve are compared bit for
bit: the reference takes every fp32 step in the kernels' order (the library is built with -ffp-contract=off), so there is
no tolerance and no excluded element.  The inputs sit on every rounding boundary of the scale and 1, 2 and 4 ulp to
either side (tests/test_projection_cpu.py states what they cover and anchors the reference to the oracle).

Above 256 levels.  The screen is derived for 256 levels: u is off by <= 1.5 lmax 2^-24 = 2.3e-5 there, the band in which it
defers to the fp64 arithmetic is 2e-4 wide, and the bound reaches the band near 2200 levels.  A numpy emulation of the
screen on the values _above_256_mismatches builds (every boundary with its ulp neighbours) gives 0 wrong levels at 257,
1024, 4096 and 16384 levels and 2214 of 593 936 at 65536, where the vector kernel would then disagree with the scalar one;
these are emulated figures, the kernels themselves were never measured above 256 levels.  The fixed points that share the
screen also tally level^2 in 32-bit integers sized for 255^2.  Every entry point that reaches the screen therefore refuses
levels > 256, as effq_admm_run and the bucket, bracket and channel entry points always did:
test_more_than_256_levels_are_refused."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.projection_ref import (F32, HAND_SCALES, ProjFused, ProjNext, host_state, projection_values, ref_project,
                                  special_values)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LEVELS = (2, 3, 4, 16, 128, 129, 255, 256)
DIVS = (1.0, 2.0, 1.25, 1.5625, 3.0)
SENTINEL = -7.25e33
GUARD = 64                                    # floats: keeps what lies between two guards 256-byte aligned
NO_OFFSET = dict(v=0, wstar=0, G=0, dual=0, Gq=0)


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_ops(DEV)


@pytest.fixture(scope="module")
def converged(ops):
    """A scale as the loop produces it: the state effq_fixed_point_small converged to on 4096 weights at 16 levels."""
    gen = torch.Generator().manual_seed(11)
    w = (torch.randn(4096, generator=gen) * 0.05).to(DEV)
    du = (torch.randn(4096, generator=gen) * 0.01).to(DEV)
    st, v = ops.new_fp_state(), torch.empty(4096, device=DEV)
    assert ops.weight_fixed_point(w, du, v, 16, st) is None
    alpha, _, done = ops.read_fp_state(st)
    assert done == 1 and 0.01 < alpha < 1.0
    return alpha, st


def _scale(which, converged):
    """(alpha, device state) of scale number `which`: the hand-written ones, then the converged one."""
    if which % 5 == 4:
        return converged
    alpha = HAND_SCALES[which % 5]
    return alpha, torch.from_numpy(host_state(alpha)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _place(host, offset, dtype=torch.float32):
    """`host` (or, for an int, that many uninitialised elements) on the device, `offset` elements past a 16-byte boundary."""
    n = host if isinstance(host, int) else host.size
    buf = torch.empty(n + offset + 16, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + n]
    if not isinstance(host, int):
        view.copy_(torch.from_numpy(host))
    return view


def _operands(alpha, levels, n, seed):
    rng = np.random.default_rng(1000 + seed)
    v = projection_values(alpha, levels, n, seed)
    wstar = (alpha * rng.standard_normal(n)).astype(F32)
    dual = (0.3 * alpha * rng.standard_normal(n)).astype(F32)
    return v, wstar, dual


def _levels_of(G, alpha, levels):
    """The level each G = f32(alpha) * f32(r d - 1) stands for (the values of distinct levels are distinct floats)."""
    d = 2.0 / float(levels - 1)
    table = F32(alpha) * (np.arange(levels, dtype=np.float64) * d + -1.0).astype(F32)
    assert np.all(np.diff(table) > 0)
    idx = np.minimum(np.searchsorted(table, G), levels - 1)
    assert np.array_equal(_bits(table[idx]), _bits(G)), "G holds values that are no level of this scale"
    return idx


def _run(ops, host, state, levels, div, want_gq, off=NO_OFFSET):
    """effq_admm_project_dual on the host operands (v, wstar, dual): (G, dual', Gq or None) as numpy arrays."""
    v, wstar, dual = host
    n = v.size
    dv, dw, dd = _place(v, off["v"]), _place(wstar, off["wstar"]), _place(dual, off["dual"])
    dG = _place(n, off["G"])
    dq = _place(n, off["Gq"], torch.int8) if want_gq else None
    for name, t in (("v", dv), ("wstar", dw), ("G", dG), ("dual", dd)):
        assert t.data_ptr() % 16 == 4 * off[name]
    if dq is not None:
        assert dq.data_ptr() % 16 == off["Gq"]
    ops.admm_project_dual(dv, dw, state, levels, dG, dd, div, dq)
    torch.cuda.synchronize()
    return dG.cpu().numpy(), dd.cpu().numpy(), (None if dq is None else dq.cpu().numpy())


def _check(got, host, alpha, levels, div):
    G, du, Gq = got
    level, G_ref, du_ref, Gq_ref, _ = ref_project(*host, alpha, levels, div)
    lv = _levels_of(G, alpha, levels)
    wrong = int(np.count_nonzero(lv != level))
    assert wrong == 0, f"{wrong} of {level.size} levels differ from the fp64 reference"
    assert np.array_equal(_bits(G), _bits(G_ref))
    assert np.array_equal(_bits(du), _bits(du_ref)), "dual"
    if Gq is not None:
        assert np.array_equal(Gq, Gq_ref), "Gq"
        # conv3d_i8s.hip: the numerator of the weight is m = Gq (Lw <= 128) or 2 Gq + 1 (Lw = 256: Gq = level - 128; in
        # between, where the conv refuses the operand, 2 Gq + 257 - Lw), the weight alpha_w m / (Lw - 1).  m is exact; G
        # rounds alpha and b to fp32 and multiplies: three roundings of <= 2^-24 alpha each
        m = Gq.astype(np.int64) if levels <= 128 else 2 * Gq.astype(np.int64) + (257 - levels)
        assert np.array_equal(m, 2 * level - (levels - 1))
        assert np.abs(G.astype(np.float64) - alpha * m / (levels - 1)).max() <= 4 * 2.0 ** -24 * alpha


# n, offsets, what
SIZE_CASES = [
    (4, {}, "vector: one group"),
    (1024, {}, "vector: one block"),
    (4100, {}, "vector: a partial last block"),
    (2097152 + 4000, {}, "vector: the grid-stride loop goes round (2048 x 256 groups per pass)"),
    (1, {}, "scalar: one element"),
    (3, {}, "scalar: n % 4 != 0"),
    (1023, {}, "scalar: n % 4 != 0, four blocks"),
    (524288 + 259, {}, "scalar: the grid-stride loop goes round"),
    (1024, {"v": 1}, "scalar: v off by one float"),
    (1024, {"wstar": 1}, "scalar: wstar off by one float"),
    (1024, {"G": 1}, "scalar: G off by one float"),
    (1024, {"dual": 1}, "scalar: dual off by one float"),
    (1024, {"Gq": 1}, "scalar: Gq off by one byte"),
]


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("case", range(len(SIZE_CASES)), ids=[f"n{c[0]}" + "".join(f"-{k}+{v}" for k, v in c[1].items())
                                                              for c in SIZE_CASES])
def test_stand_alone_projection_equals_the_reference(ops, converged, levels, case):
    n, shift, _ = SIZE_CASES[case]
    alpha, state = _scale(case + levels, converged)
    div = DIVS[(case + levels) % len(DIVS)]
    host = _operands(alpha, levels, n, seed=case)
    off = dict(NO_OFFSET, **shift)
    for want_gq in ((True,) if "Gq" in shift else (True, False)):
        got = _run(ops, host, state, levels, div, want_gq, off)
        _check(got, host, alpha, levels, div)
        if shift:                                        # ... and the scalar kernel equals the vector kernel
            ref = _run(ops, host, state, levels, div, want_gq)
            assert np.array_equal(_bits(got[0]), _bits(ref[0])) and np.array_equal(_bits(got[1]), _bits(ref[1]))
            assert want_gq is False or np.array_equal(got[2], ref[2])


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("which", range(5), ids=[f"alpha{a:g}" for a in HAND_SCALES] + ["converged"])
def test_every_scale_at_every_level_count_on_both_kernels(ops, converged, levels, which):
    """n = 4100 holds every special value of 256 levels (about 2700); 4099 of the same values take the scalar kernel."""
    alpha, state = _scale(which, converged)
    assert special_values(alpha, levels, 0).size < 4099
    host = _operands(alpha, levels, 4100, seed=which)
    _check(_run(ops, host, state, levels, 1.5625, True), host, alpha, levels, 1.5625)
    host = tuple(a[:4099] for a in host)
    _check(_run(ops, host, state, levels, 1.5625, True), host, alpha, levels, 1.5625)


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("n", [4100, 4099], ids=["vector", "scalar"])
def test_dual_divisors(ops, converged, div, n):
    """1 (no division), "dual /= 2", and rho_m / rho = 1.25, 1.5625, 3: the dual bit for bit, the quotient rounded once."""
    for levels in (4, 256):
        alpha, state = _scale(4, converged)
        host = _operands(alpha, levels, n, seed=int(div * 10000))
        got = _run(ops, host, state, levels, div, False)
        _check(got, host, alpha, levels, div)
        _, G_ref, du_ref, _, _ = ref_project(*host, alpha, levels, div)
        undivided = (host[1] - G_ref) + host[2]
        assert np.array_equal(_bits(got[1]), _bits(undivided / F32(div)))
        assert (div == 1.0) == np.array_equal(_bits(got[1]), _bits(undivided))


def test_int8_numerators_are_refused_above_256_levels(ops):
    from efficientq_amd._lib import EffqError
    alpha = 0.73
    host = _operands(alpha, 257, 1024, seed=0)
    state = torch.from_numpy(host_state(alpha)).to(DEV)
    with pytest.raises(EffqError):
        _run(ops, host, state, 257, 1.0, True)


def _above_256_mismatches(ops, levels, offset):
    """Wrong levels of the stand-alone projection on the boundary values of `levels` levels (Gq = None): aligned operands
    (offset 0: the vector kernel) or all four off by one float (the scalar kernel).  (count, n)"""
    alpha = 0.0371234567
    n = -(-(special_values(alpha, levels, 0).size + 4096) // 4) * 4
    host = _operands(alpha, levels, n, seed=levels)
    state = torch.from_numpy(host_state(alpha)).to(DEV)
    G, du, _ = _run(ops, host, state, levels, 1.0, False, dict(v=offset, wstar=offset, G=offset, dual=offset, Gq=0))
    level = ref_project(*host, alpha, levels, 1.0)[0]
    return int(np.count_nonzero(_levels_of(G, alpha, levels) != level)), n


@pytest.mark.parametrize("levels", [257, 1024, 4096, 65536])
def test_more_than_256_levels_are_refused(ops, levels):
    """(See the module docstring for what the kernels did with them.)  The projection on either kernel, and the weight and
    activation fixed points whose statistics passes use the same screen."""
    from efficientq_amd._lib import EffqError, check
    from efficientq_amd.hip_ops import ADMM_TOL
    for offset in (0, 1):
        with pytest.raises(EffqError):
            _above_256_mismatches(ops, levels, offset)
    lib = ops.lib
    small, coop = 4096, int(lib.effq_fp_small_max()) + 4096
    for n in (small, coop):
        w, du, v = (torch.zeros(n, device=DEV) + 0.01 for _ in range(3))
        with pytest.raises(EffqError):
            ops.weight_fixed_point(w, du, v, levels, ops.new_fp_state())
    with pytest.raises(EffqError):
        ops.fixed_point_coop_rec(w, du, v, levels, ops.new_fp_state(), ops.new_fp_pred())
    x, st = torch.rand(4096, device=DEV), ops.new_fp_state()
    with pytest.raises(EffqError):
        ops.fit_scale(x, levels, 0.0, 1.0)
    with pytest.raises(EffqError):
        check(lib.effq_alpha_stats_f64(x.data_ptr(), st.data_ptr(), 0.0, 1.0, levels, x.numel(), st[2:4].data_ptr(), None,
                                       ops._red_ws.data_ptr(), ops.stream), "effq_alpha_stats_f64")
    with pytest.raises(EffqError):
        check(lib.effq_alpha_fixed_point(x.data_ptr(), x.numel(), levels, 0.0, 1.0, ADMM_TOL, 100, 4, st.data_ptr(),
                                         ops._red_ws.data_ptr(), ops.stream), "effq_alpha_fixed_point")
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the next right-hand side and the fused epilogue
# c2, nwrow, has_bias
# (k_fp_small runs 256 threads up to 2048 values, 512 up to 16384, else 1024: 64 x 64 takes 512, hence the last shape)
SHAPES = [(8, 32, 1), (8, 27, 1), (64, 64, 0), (48, 108, 1), (32, 864, 1), (16, 128, 0)]
SHAPE_IDS = ["8x32-vector", "8x27-scalar", "64x64-512-threads", "48x108-512-threads", "32x864-1024-threads",
             "16x128-256-threads"]
RHO, ETA = 37.3, 3.3                          # neither is an fp32 value


def _impl(lib):
    fn = lib.effq_project_dual_impl
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t,
                   C.c_void_p, C.POINTER(ProjNext), C.c_void_p]
    return fn


def _fused(lib):
    fn = lib.effq_fixed_point_small_fused
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                   C.c_void_p, C.POINTER(ProjFused), C.c_void_p]
    return fn


def test_struct_mirrors_have_the_layout_of_project_dual_h():
    assert C.sizeof(ProjNext) == 48 and C.sizeof(ProjFused) == 112


class _Next:
    """B0, W0 and a sentinel-filled Bm between guards for a (c2, nwrow, has_bias) layer, with the ProjNext that names them."""

    def __init__(self, c2, nwrow, has_bias, seed):
        rng = np.random.default_rng(seed)
        self.c2, self.nwrow, self.n = c2, nwrow, nwrow + has_bias
        self.ldb = -(-self.n // 4) * 4
        self.B0 = rng.standard_normal((c2, self.n)).astype(F32)
        self.W0 = (0.1 * rng.standard_normal(c2 * nwrow)).astype(F32)
        self.dB0, self.dW0 = torch.from_numpy(self.B0).to(DEV), _place(self.W0, 0)
        self.buf = torch.full((c2 * self.ldb + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.dBm = self.buf[GUARD:GUARD + c2 * self.ldb]
        assert self.dBm.data_ptr() % 16 == 0 and self.dW0.data_ptr() % 16 == 0
        self.struct = ProjNext(self.dBm.data_ptr(), self.dB0.data_ptr(), self.dW0.data_ptr(), nwrow, self.n, self.ldb,
                               RHO, ETA)

    def as_ref(self):
        return dict(B0=self.B0, W0=self.W0, nwrow=self.nwrow, n=self.n, ldb=self.ldb, rho=RHO, eta=ETA, fill=F32(SENTINEL))

    def check(self, Bm_ref):
        buf = self.buf.cpu().numpy()
        assert np.all(buf[:GUARD] == F32(SENTINEL)) and np.all(buf[-GUARD:] == F32(SENTINEL)), "written outside Bm"
        Bm = buf[GUARD:-GUARD].reshape(self.c2, self.ldb)
        assert np.all(Bm[:, self.nwrow:] == F32(SENTINEL)), "the bias column or the padding of Bm was written"
        assert np.array_equal(_bits(Bm[:, :self.nwrow]), _bits(Bm_ref[:, :self.nwrow])), "weight columns of Bm"


@pytest.mark.parametrize("levels", [4, 16, 256])
@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=SHAPE_IDS)
def test_projection_that_writes_the_next_right_hand_side(ops, converged, shape, levels):
    """effq_project_dual_impl with nx != NULL on the vector kernel (rows of a multiple of 4) and the scalar one (rows of
    27): Bm's weight columns are (B0 + eta W0) + rho (G - the NEW dual), its bias column and padding are not touched, and
    the folded-in convergence check leaves err_flag at 0 for a converged state."""
    c2, nwrow, has_bias = SHAPES[shape]
    nw = c2 * nwrow
    alpha, state = _scale(shape + levels, converged)
    div = DIVS[(shape + 1) % len(DIVS)]
    host = _operands(alpha, levels, nw, seed=shape)
    nx = _Next(c2, nwrow, has_bias, seed=shape)
    dv, dw, dd, dG, dq = _place(host[0], 0), _place(host[1], 0), _place(host[2], 0), _place(nw, 0), _place(nw, 0, torch.int8)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _impl(ops.lib)(dv.data_ptr(), dw.data_ptr(), state.data_ptr(), levels, dG.data_ptr(), dd.data_ptr(), div,
                        dq.data_ptr(), nw, err.data_ptr(), C.byref(nx.struct), ops.stream)
    assert rc == 0
    torch.cuda.synchronize()
    _check((dG.cpu().numpy(), dd.cpu().numpy(), dq.cpu().numpy()), host, alpha, levels, div)
    nx.check(ref_project(*host, alpha, levels, div, nx.as_ref())[4])
    assert int(err.item()) == 0


@pytest.mark.parametrize("shape", [0, 1], ids=SHAPE_IDS[:2])
@pytest.mark.parametrize("done,flag", [(1, 0), (2, 2), (0, 3)])
def test_folded_in_convergence_check(ops, shape, done, flag):
    """err_flag of the stand-alone kernels: untouched for done = 1, 2 at the iteration cap, 3 for anything else."""
    c2, nwrow, has_bias = SHAPES[shape]
    nw, alpha, levels = c2 * nwrow, 0.73, 4
    host = _operands(alpha, levels, nw, seed=shape)
    state = torch.from_numpy(host_state(alpha, iters=400, done=done)).to(DEV)
    nx = _Next(c2, nwrow, has_bias, seed=shape)
    dv, dw, dd, dG = _place(host[0], 0), _place(host[1], 0), _place(host[2], 0), _place(nw, 0)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _impl(ops.lib)(dv.data_ptr(), dw.data_ptr(), state.data_ptr(), levels, dG.data_ptr(), dd.data_ptr(), 1.0, None,
                        nw, err.data_ptr(), C.byref(nx.struct), ops.stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(err.item()) == flag
    _check((dG.cpu().numpy(), dd.cpu().numpy(), None), host, alpha, levels, 1.0)     # the projection runs all the same


@pytest.mark.parametrize("levels", [4, 16, 256])
@pytest.mark.parametrize("shape", [2, 3, 4, 5], ids=SHAPE_IDS[2:])
def test_fused_epilogue_equals_the_reference(ops, shape, levels):
    """effq_fixed_point_small_fused as effq_admm_run calls it (a = w*, b = dual, the epilogue projects v = w* + dual at the
    scale the same launch converged to): one launch of k_fp_small with 256, 512 and 1024 threads."""
    from efficientq_amd.hip_ops import ADMM_TOL
    c2, nwrow, has_bias = SHAPES[shape]
    nw = c2 * nwrow
    assert nw % 4 == 0 and nwrow % 4 == 0 and nw <= ops.lib.effq_fp_small_max()
    assert (256 if nw <= 2048 else 512 if nw <= 16384 else 1024) == int(SHAPE_IDS[shape].split("-")[1])
    rng = np.random.default_rng(shape + levels)
    wstar = (0.05 * rng.standard_normal(nw)).astype(F32)
    dual = (0.01 * rng.standard_normal(nw)).astype(F32)
    div = DIVS[(shape + levels) % len(DIVS)]
    nx = _Next(c2, nwrow, has_bias, seed=shape)
    dw, dd, dv, dG, dq = _place(wstar, 0), _place(dual, 0), _place(nw, 0), _place(nw, 0), _place(nw, 0, torch.int8)
    err, st = torch.zeros(1, dtype=torch.int32, device=DEV), ops.new_fp_state()
    pf = ProjFused(dw.data_ptr(), dG.data_ptr(), dd.data_ptr(), dq.data_ptr(), err.data_ptr(), 2.0 / float(levels - 1), div,
                   levels - 1, nw // 4, nx.struct)
    rc = _fused(ops.lib)(dw.data_ptr(), dd.data_ptr(), dv.data_ptr(), nw, levels, -1.0, 1.0, ADMM_TOL, 100 * levels,
                         st.data_ptr(), C.byref(pf), ops.stream)
    assert rc == 0
    torch.cuda.synchronize()
    alpha, iters, done = ops.read_fp_state(st)
    assert done == 1 and iters >= 2 and int(err.item()) == 0
    v = wstar + dual
    assert np.array_equal(_bits(dv.cpu().numpy()), _bits(v))
    host = (v, wstar, dual)
    _check((dG.cpu().numpy(), dd.cpu().numpy(), dq.cpu().numpy()), host, alpha, levels, div)
    nx.check(ref_project(*host, alpha, levels, div, nx.as_ref())[4])
    # the stand-alone vector kernel on the same operands and state: the same bits
    got = _run(ops, host, st, levels, div, True)
    assert np.array_equal(_bits(got[0]), _bits(dG.cpu().numpy())) and np.array_equal(_bits(got[1]), _bits(dd.cpu().numpy()))
