"""The gradient path behind tune_activation_range (row f3), kernel by kernel against fp64.

  A  effq_act_quant_backward (k_act_quant_bwd): the straight-through backward of the activation quantiser
  B  effq_adam_step (k_adam)
  C  PTQConv._dgrad (the conv kernel on the output gradient with flipped, transposed weights) and _QuantConvFn
  D  one step of the driver on a two-conv model

The end-to-end test of test_layer_gpu.py allows 2e-3 after 50 steps that move an alpha by at most lr each, whatever the
gradient: it cannot see a wrong clamp mask at u == 0 or u == 1, a tie rounded the wrong way, a dropped grid-stride tail, a
stale reduction ticket or a transposition slip that keeps the loss falling.  Every tolerance here is derived from the
roundings of the arithmetic under test or is the 1e-5 that test_conv_tiles_gpu.py uses for the fp32 conv kernels against
fp64; the derivations stand next to the bounds.

References are computed on the CPU (numpy / torch, fp64, or fp32 where the kernel's own fp32 arithmetic is restated).
Runs on a real MI355X only (-m gpu)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TPB, RED_MAX_BLOCKS = 256, 2048                 # csrc/common.h: the streaming kernels' block size and grid cap
BIG = RED_MAX_BLOCKS * TPB + 257                # the capped grid walks the array twice and ends in a ragged tail
F32, F64 = np.float32, np.float64
MIN_NORMAL = F32(1.1754943508222875e-38)


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_ops(DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# =================================================================== A. effq_act_quant_backward
# The kernel, in fp32 without contraction: u = x / alpha, c = clamp(u, 0, 1), r = rint(c / d) * d, m = [0 <= u <= 1],
# gx = g * m, galpha = sum of fl32(g * fl32(r - m * u)) accumulated in double, d = float(1 / (L - 1)).
LEVELS = (2, 4, 16, 256)
SIZES = (1, 255, 257, 70001, BIG)
ALPHAS = (0.37, 0.5, 2.0)
EDGE_NAMES = ("alpha", "above_alpha", "zero", "neg_zero", "below_zero", "neg_min_normal")


def _edge_points(alpha):
    a = F32(alpha)
    return [a, np.nextafter(a, F32(np.inf)), F32(0.0), F32(-0.0), np.nextafter(F32(0.0), F32(-np.inf)), -MIN_NORMAL]


def _boundary_points(alpha, levels):
    """(k - 0.5) * d * alpha for up to 8 values of k spread over 1 .. L-1, and one ulp either side of each."""
    a, d = F32(alpha), F32(1.0 / (levels - 1))
    pts = []
    for k in np.unique(np.linspace(1, levels - 1, 8).round()):
        b = F32(k - 0.5) * d * a
        pts += [np.nextafter(b, F32(-np.inf)), b, np.nextafter(b, F32(np.inf))]
    return pts


def _quant_inputs(n, alpha, levels, seed, boundaries=True):
    """x = relu(randn + 0.2) * alpha (about 42 % exact zeros, 21 % above alpha) with one value in ten negative, g = randn,
    and - from 64 elements on - the planted points at random places.  Returns x, g and the places of the edge points."""
    rng = np.random.default_rng(seed)
    a = F32(alpha)
    x = np.maximum(rng.standard_normal(n).astype(F32) + F32(0.2), F32(0.0)) * a
    neg = rng.random(n) < 0.1
    x[neg] = -np.abs(rng.standard_normal(int(neg.sum())).astype(F32)) * a
    g = rng.standard_normal(n).astype(F32)
    where = {}
    if n >= 64:
        pts = _edge_points(alpha) + (_boundary_points(alpha, levels) if boundaries else [])
        pos = rng.permutation(n)[:len(pts)]
        x[pos] = np.array(pts, dtype=F32)
        where = dict(zip(EDGE_NAMES, pos[:len(EDGE_NAMES)].tolist()))
    return x, g, where


def _bwd_ref32(x, g, alpha, levels):
    """The kernel's fp32 arithmetic restated with IEEE operations on the CPU; the sum in fp64.
    Returns gx (fp32), galpha (fp64), sum |term| (fp64) and the mask."""
    a, d = F32(alpha), F32(1.0 / (levels - 1))
    u = x / a
    c = np.minimum(np.maximum(u, F32(0.0)), F32(1.0))
    r = np.rint(c / d) * d
    m = ((u >= 0) & (u <= 1)).astype(F32)
    assert u.dtype == r.dtype == F32
    terms = g.astype(F64) * (r.astype(F64) - m.astype(F64) * u.astype(F64))
    return g * m, float(terms.sum()), float(np.abs(terms).sum()), m


def _run_bwd(ops, x, g, alpha, levels, want_gx=True, shape=None):
    xt, gt = _dev(x), _dev(g)
    if shape is not None:
        xt, gt = xt.reshape(shape), gt.reshape(shape)
    gx, ga = ops.act_quant_backward(xt, torch.tensor(alpha, dtype=torch.float32, device=DEV), levels, gt, want_gx=want_gx)
    assert ga.dtype == torch.float64 and ga.numel() == 1
    if gx is not None:
        assert gx.shape == xt.shape and gx.dtype == torch.float32
        gx = gx.cpu().numpy().reshape(-1)
    return gx, ga.cpu().item()


def _check_bwd(ops, x, g, alpha, levels, shape=None):
    """Checks A.1 and A.2 for one call; returns (gx, galpha) of the kernel."""
    gx_ref, ga_ref, abs_sum, _ = _bwd_ref32(x, g, alpha, levels)
    gx, ga = _run_bwd(ops, x, g, alpha, levels, shape=shape)
    bad = np.flatnonzero(_bits(gx) != _bits(gx_ref))
    assert bad.size == 0, (bad.size, bad[:5], x[bad[:5]], gx[bad[:5]], gx_ref[bad[:5]])
    # every term carries two fp32 roundings (the subtraction and the product; m * u is exact): 2 * 2^-24 of its size
    assert abs(ga - ga_ref) <= 2.0 ** -23 * abs_sum, (ga, ga_ref, abs(ga - ga_ref), 2.0 ** -23 * abs_sum)
    return gx, ga


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("levels", LEVELS)
def test_act_quant_backward_matches_its_fp32_arithmetic(ops, levels, n):
    """A.1: gx is bitwise g * m, with m from the IEEE fp32 quotient x / alpha and both bounds included - m = 1 at x = 0,
    -0.0 and alpha, m = 0 one ulp outside either bound.  A.2: galpha against the same fp32 terms summed in fp64, within
    2^-23 * sum |g (r - m u)|.  Sizes: one element, one block short of and past full, several blocks, and the capped grid
    taking a second trip with a ragged tail."""
    for alpha in ALPHAS:
        x, g, where = _quant_inputs(n, alpha, levels, seed=1000 * levels + n % 997)
        if where:
            m = _bwd_ref32(x, g, alpha, levels)[3]
            want = dict(alpha=1, above_alpha=0, zero=1, neg_zero=1, neg_min_normal=0)
            # the smallest negative number divided by an alpha above 1 rounds to -0.0, which is inside the bounds
            want["below_zero"] = 0 if alpha <= 1 else 1
            assert {k: int(m[i]) for k, i in where.items()} == want, alpha
        _check_bwd(ops, x, g, alpha, levels)


def test_act_quant_backward_takes_the_5d_ndhwc_tensor(ops):
    """The call of qconv.py: x and gq as contiguous (N, D, H, W, C) tensors; gx comes back in that shape."""
    shape = (2, 5, 6, 7, 16)
    x, g, _ = _quant_inputs(int(np.prod(shape)), 0.37, 4, seed=5)
    _check_bwd(ops, x, g, 0.37, 4, shape=shape)


class _RoundSTE(torch.autograd.Function):
    """round with identity gradient (the reference's RoundDifferentiable)."""

    @staticmethod
    def forward(ctx, x):
        return x.round()

    @staticmethod
    def backward(ctx, g):
        return g


def _quant64(x, alpha, levels):
    """The reference's five operations: divide, clamp, affine, round (identity gradient), affine and multiply by alpha."""
    d = 1.0 / (levels - 1)
    return (_RoundSTE.apply((torch.clamp(x / alpha, 0.0, 1.0) - 0.0) / d) * d + 0.0) * alpha


def _near_half(x64, alpha, levels, margin=1e-3):
    """Inputs whose c / d lies within `margin` of a half-integer: the side the rounding falls on may differ between d in
    fp32 and in fp64 there."""
    v = np.clip(x64 / alpha, 0.0, 1.0) * (levels - 1)
    return np.abs(v - np.floor(v) - 0.5) < margin


@pytest.mark.parametrize("alpha", (0.5, 2.0))
@pytest.mark.parametrize("levels", LEVELS)
def test_act_quant_backward_formula_vs_fp64_autograd(ops, levels, alpha):
    """A.3: galpha and gx against fp64 autograd through the reference's five operations.  alpha is a power of two, so u is
    exact in both precisions; inputs within 1e-3 of a rounding boundary are removed (at most 1 %).  Bound on galpha:
    2^-22 * sum |g| (|r| + |u|) - four fp32 roundings per term (d itself, r = k * d, the subtraction, the product).  gx
    against autograd's g * alpha * d / d * m / alpha: two fp64 roundings, 2^-51 |g| with the second-order terms."""
    n = 70001
    x, g, _ = _quant_inputs(n, alpha, levels, seed=77 + levels, boundaries=False)
    # (and the planted denormal: its fp32 quotient by an alpha above 1 is not exact - it rounds to -0.0)
    drop = _near_half(x.astype(F64), alpha, levels) | ((x != 0) & (np.abs(x) < MIN_NORMAL))
    assert drop.mean() <= 0.01, drop.mean()
    x, g = x[~drop], g[~drop]
    xt = torch.tensor(x.astype(F64), requires_grad=True)
    at = torch.tensor(float(alpha), dtype=torch.float64, requires_grad=True)
    (_quant64(xt, at, levels) * torch.tensor(g.astype(F64))).sum().backward()
    u = x.astype(F64) / alpha
    r = np.rint(np.clip(u, 0.0, 1.0) * (levels - 1)) / (levels - 1)
    bound = 2.0 ** -22 * float((np.abs(g.astype(F64)) * (np.abs(r) + np.abs(u))).sum())
    gx, ga = _run_bwd(ops, x, g, alpha, levels)
    assert abs(ga - at.grad.item()) <= bound, (ga, at.grad.item(), abs(ga - at.grad.item()), bound)
    assert np.all(np.abs(gx.astype(F64) - xt.grad.numpy()) <= 2.0 ** -51 * np.abs(g.astype(F64)))


@pytest.mark.parametrize("alpha", (0.5, 2.0))
@pytest.mark.parametrize("levels", (2, 5, 17))
def test_act_quant_backward_rounds_ties_to_even(ops, levels, alpha):
    """A.4: 1000 inputs exactly on rounding ties u = (k + 0.5) d (d and alpha powers of two: every operation is exact) with
    g = 1 on a background of zeros.  galpha equals the round-half-to-even value exactly; rounding half away from zero
    would differ by d at every tie whose lower neighbour is even."""
    n, nt = 70001, 1000
    rng = np.random.default_rng(levels)
    d = 1.0 / (levels - 1)
    k = rng.integers(0, levels - 1, nt)
    u = (k + 0.5) * d
    pos = rng.permutation(n)[:nt]
    x, g = np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
    x[pos], g[pos] = (u * alpha).astype(F32), F32(1.0)
    assert np.all(x[pos].astype(F64) == u * alpha)
    even = float((np.rint(k + 0.5) * d - u).sum())              # numpy rounds half to even
    away = float((np.floor(k + 0.5 + 0.5) * d - u).sum())
    assert even != away
    _, ga = _run_bwd(ops, x, g, alpha, levels)
    assert ga == even, (ga, even, away)


def test_act_quant_backward_call_variants_and_errors(ops):
    """A.5: want_gx=False gives no gx and the same galpha bit for bit; a repeated call repeats its results bit for bit; two
    different calls back to back on one ops each match their own reference (the last block rearms the reduction ticket);
    one level and an empty tensor are refused."""
    from efficientq_amd._lib import EffqError
    xa, ga_in, _ = _quant_inputs(70001, 0.37, 16, seed=1)
    xb, gb_in, _ = _quant_inputs(BIG, 2.0, 4, seed=2)
    gx1, ga1 = _check_bwd(ops, xa, ga_in, 0.37, 16)
    _check_bwd(ops, xb, gb_in, 2.0, 4)                       # 2048 blocks right after 274: a stale ticket would show here
    gx2, ga2 = _check_bwd(ops, xa, ga_in, 0.37, 16)          # ... or here
    assert ga2 == ga1 and np.array_equal(_bits(gx2), _bits(gx1))
    none, ga3 = _run_bwd(ops, xa, ga_in, 0.37, 16, want_gx=False)
    assert none is None and ga3 == ga1
    with pytest.raises(EffqError):
        _run_bwd(ops, xa, ga_in, 0.37, 1)
    with pytest.raises(EffqError):
        _run_bwd(ops, xa[:0], ga_in[:0], 0.37, 4)
    _check_bwd(ops, xa[:257], ga_in[:257], 0.37, 16)         # the refused calls left the workspace usable


# =================================================================== B. effq_adam_step
LR, B1, B2, EPS = 5e-4, 0.9, 0.999, 1e-8         # the defaults of tune.py and of the reference's Adam(opt_param, lr=5e-4)
ADAM_FACTOR = 4.0


def _adam64(p, m, v, g, t):
    """Adam (no weight decay, no amsgrad) in fp64 with Python-double betas, in place."""
    m *= B1
    m += (1 - B1) * g
    v *= B2
    v += (1 - B2) * g * g
    p -= LR * (m / (1 - B1 ** t)) / (np.sqrt(v / (1 - B2 ** t)) + EPS)


def _adam_problem(n, seed, p_lo=0.25):
    """p0 log-uniform in [p_lo, 4]; gradient scales 1, 1e6, 1e-12 in turn; the elements 3, 10, 17, ... get a zero gradient
    at every step.  Over a trajectory p0 stays at or above 0.25, where the alphas of the nets lie: a step is at most
    lr * max(1, (1 - b1) / sqrt(1 - b2)) = 3.2 lr long, 60 of them 0.095, so no parameter comes near zero, where ulp32(p64)
    collapses under the rounding errors gathered at the earlier size of p and the yardstick turns into the ratio of two
    such errors - unbounded for any two fp32 evaluation orders."""
    rng = np.random.default_rng(seed)
    p0 = np.exp(rng.uniform(np.log(p_lo), np.log(4.0), n)).astype(F32)
    scale = np.array([1.0, 1e6, 1e-12], dtype=F32)[np.arange(n) % 3]
    scale[np.arange(n) % 7 == 3] = 0.0
    return rng, p0, scale


class _Torch32:
    """torch.optim.Adam on CPU fp32 tensors: the reference project's optimiser, and the yardstick."""

    def __init__(self, p0, t0=0):
        self.p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        self.opt = torch.optim.Adam([self.p], lr=LR, betas=(B1, B2), eps=EPS)
        if t0:
            self.opt.state[self.p] = dict(step=torch.tensor(float(t0)), exp_avg=torch.zeros_like(self.p.data),
                                          exp_avg_sq=torch.zeros_like(self.p.data))

    def step(self, g):
        self.p.grad = torch.from_numpy(g.copy())
        self.opt.step()
        return self.p.detach().numpy().astype(F64)


def _adam_ratio(p_kernel, p_torch, p64):
    """Elementwise |p_kernel - p64| over max(|p_torch32 - p64|, ulp32(p64)); returns the worst."""
    ulp = np.spacing(np.abs(p64).astype(F32)).astype(F64)
    yard = np.maximum(np.abs(p_torch - p64), ulp)
    return float((np.abs(p_kernel.astype(F64) - p64) / yard).max())


@pytest.mark.parametrize("n", (1, 23, 257, BIG))
def test_adam_step_follows_the_fp64_trajectory(ops, n):
    """B: 60 consecutive steps (t = 1 .. 60, a fresh randn gradient each, scales 1e-12, 1 and 1e6) against Adam in fp64
    with Python-double betas.  After every step |p_kernel - p64| <= 4 * max(|p_torch32 - p64|, ulp32(p64)) elementwise,
    torch.optim.Adam on CPU fp32 tensors being the yardstick and 4 the allowance for another legitimate fp32 evaluation
    order.  Elements whose gradient is zero at every step keep p, m and v bit for bit (tune.py relies on it for unused
    alphas).

    Measured with an IEEE fp32 restatement of the kernel's arithmetic on the CPU, worst ratio over all steps and elements:
    1.0, 1.0, 1.0 and 2.99 for the four sizes.  The kernel as it stood before this test - betas as floats, 1 - powf(b, t)
    in fp32 - gave 1.0, 1.0, 2.0 and 3.997 here: inside the yardstick on a trajectory, by a hair; it is the single steps
    at large t below that it missed."""
    rng, p0, scale = _adam_problem(n, seed=n)
    still = scale == 0
    p64, m64, v64 = p0.astype(F64), np.zeros(n), np.zeros(n)
    ref32 = _Torch32(p0)
    p, m, v = _dev(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    worst = 0.0
    for t in range(1, 61):
        g = rng.standard_normal(n).astype(F32) * scale
        ops.adam_step(p, _dev(g), m, v, LR, t)
        _adam64(p64, m64, v64, g.astype(F64), t)
        pk = p.cpu().numpy()
        worst = max(worst, _adam_ratio(pk, ref32.step(g), p64))
        assert np.array_equal(_bits(pk[still]), _bits(p0[still])), t
    print(f"adam n={n}: worst |p_kernel - p64| / max(|p_torch32 - p64|, ulp32) over 60 steps = {worst:.3f}")
    assert worst <= ADAM_FACTOR, worst
    assert not m.cpu().numpy()[still].any() and not v.cpu().numpy()[still].any()
    assert np.array_equal(_bits(m.cpu().numpy()[still]), np.zeros(int(still.sum()), dtype=np.int32))
    assert np.array_equal(_bits(v.cpu().numpy()[still]), np.zeros(int(still.sum()), dtype=np.int32))


@pytest.mark.parametrize("t", (1000, 100000))
def test_adam_step_bias_corrections_at_large_t(ops, t):
    """B: one step at t = 1000 and t = 100000 from fresh zero moments: the bias corrections 1 - beta^t as the fp64
    reference forms them, under the same yardstick.  p0 reaches down to 1e-3 and is 0 at every fifth element: there
    p_new is of the size of the step, whose relative error is then not hidden under the rounding of p.

    Measured with the same restatement: 1.79 at t = 1000, 2.31 at t = 100000.  With the betas as floats it was 125 and
    219: 1 - (float)0.999 is 1.3e-5 off 1 - 0.999 and no longer cancels against 1 - beta2^t, so effq_adam_step now takes
    doubles and forms the corrections in double on the host."""
    n = 257
    rng, p0, scale = _adam_problem(n, seed=t, p_lo=1e-3)
    p0[::5] = 0.0           # there p_new is the step itself: its relative error is not hidden under the rounding of p
    g = rng.standard_normal(n).astype(F32) * scale
    p64, m64, v64 = p0.astype(F64), np.zeros(n), np.zeros(n)
    _adam64(p64, m64, v64, g.astype(F64), t)
    p_torch = _Torch32(p0, t0=t - 1).step(g)
    p, m, v = _dev(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ops.adam_step(p, _dev(g), m, v, LR, t)
    ratio = _adam_ratio(p.cpu().numpy(), p_torch, p64)
    print(f"adam t={t}: |p_kernel - p64| / max(|p_torch32 - p64|, ulp32) = {ratio:.3f}")
    assert ratio <= ADAM_FACTOR, ratio


@pytest.mark.parametrize("n", (23, BIG))
def test_adam_first_step_moves_by_lr(ops, n):
    """B: at t = 1 the bias corrections cancel the moments' weights: p_new - p_old = -lr * g / (|g| + eps).  From p = 0 (so
    that p_new is the step itself, free of the rounding of p), wherever |g| >= 1e-3: -lr * sign(g) within lr * 2e-5 -
    eps / |g| <= 1e-5 relative, the fp32 roundings of the step about 1e-6 more."""
    rng = np.random.default_rng(n)
    g = rng.standard_normal(n).astype(F32) * np.array([1.0, 1e6, 1e-2], dtype=F32)[np.arange(n) % 3]
    p, m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ops.adam_step(p, _dev(g), m, v, LR, 1)
    big = np.abs(g) >= 1e-3
    assert big.mean() > 0.6
    step = p.cpu().numpy().astype(F64)[big]
    assert np.all(np.abs(step + LR * np.sign(g[big])) <= LR * 2e-5), np.abs(step + LR * np.sign(g[big])).max() / LR


def test_adam_step_errors(ops):
    """B: t = 0 is refused; an empty parameter vector is a no-op."""
    from efficientq_amd._lib import EffqError
    p, g = torch.ones(5, device=DEV), torch.ones(5, device=DEV)
    m, v = torch.zeros(5, device=DEV), torch.zeros(5, device=DEV)
    with pytest.raises(EffqError):
        ops.adam_step(p, g, m, v, LR, 0)
    assert p.cpu().tolist() == [1.0] * 5 and not m.cpu().numpy().any() and not v.cpu().numpy().any()
    e = torch.empty(0, device=DEV)
    ops.adam_step(e, e.clone(), e.clone(), e.clone(), LR, 1)
    torch.cuda.synchronize()


# =================================================================== C. PTQConv._dgrad and _QuantConvFn
N_C, SP_C = 2, (5, 6, 7)
CONV_CASES = {
    # id: (c_in, c_out, kernel, padding); c_in != c_out everywhere: a flip or transposition slip cannot hide
    "k3_16to32": (16, 32, 3, 1),
    "k3_32to16": (32, 16, 3, 1),
    "k1_32to3_classifier": (32, 3, 1, 0),            # its gradient conv has 3 input channels
    "k1_64to32": (64, 32, 1, 0),
    "k133_16to32": (16, 32, (1, 3, 3), (0, 1, 1)),
}


def _module(c1, c2, k, pad, seed, stride=1, q_act=True, levels=4, alpha=0.5):
    """A PTQConv in quantised mode with random (not symmetric) weights; returns it with its fp64 weights and bias."""
    from efficientq_amd.qconv import PTQConv
    gen = torch.Generator().manual_seed(seed)
    mod = PTQConv(c1, c2, k, stride, pad, bias=True, q_act=q_act, qlvl_act=levels)
    with torch.no_grad():
        mod.weight.copy_(torch.randn(mod.weight.shape, generator=gen) / float(np.sqrt(mod.weight[0].numel())))
        mod.bias.copy_(torch.randn(c2, generator=gen) * 0.1)
        mod.alpha_act.fill_(alpha)
    mod.to(DEV)
    mod.set_quantized()
    return mod, mod.weight.detach().cpu().double(), mod.bias.detach().cpu().double()


def _act_input(shape, alpha, levels, seed):
    """The inputs of A on a conv's input grid, values within 1e-3 of a rounding boundary (and the planted
    denormal) replaced by 0 (at most 1 %)."""
    x, _, _ = _quant_inputs(int(np.prod(shape)), alpha, levels, seed, boundaries=False)
    drop = _near_half(x.astype(F64), alpha, levels) | ((x != 0) & (np.abs(x) < MIN_NORMAL))    # as in A.3
    assert drop.mean() <= 0.01, drop.mean()
    x[drop] = 0.0
    return torch.from_numpy(x).reshape(shape)


def _conv_ref(x, w, b, pad, g, alpha=None, levels=0):
    """fp64 autograd through [the five-operation quantiser and] F.conv3d: (gx, galpha or None, gq, bound on galpha)."""
    xt = x.double().requires_grad_(True)
    if alpha is None:
        F.conv3d(xt, w, b, 1, pad).backward(g.double())
        return xt.grad, None, None, None
    at = torch.tensor(float(alpha), dtype=torch.float64, requires_grad=True)
    q = _quant64(xt, at, levels)
    q.retain_grad()
    F.conv3d(q, w, b, 1, pad).backward(g.double())
    u = x.double() / alpha
    m = ((u >= 0) & (u <= 1)).double()
    r = torch.round(torch.clamp(u, 0.0, 1.0) * (levels - 1)) / (levels - 1)
    # the bound of A.2 on the sum, and the conv's 1e-5 * max |gq| on every gq carried through the sum
    bound = 2.0 ** -23 * (q.grad * (r - m * u)).abs().sum().item() \
        + 1e-5 * q.grad.abs().max().item() * (r - m * u).abs().sum().item()
    return xt.grad, at.grad.item(), q.grad, bound


def _grad_out(mod, seed):
    return torch.randn(N_C, mod.out_channels, *SP_C, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("case", list(CONV_CASES))
def test_dgrad_matches_fp64_autograd(ops, case):
    """The conv kernel on the output gradient with flipped, transposed weights against fp64 autograd through F.conv3d:
    max |gx - ref| <= 1e-5 * max |ref|, the figure of test_conv_tiles_gpu.py for the same fp32 kernels."""
    c1, c2, k, pad = CONV_CASES[case]
    mod, w, b = _module(c1, c2, k, pad, seed=len(case))
    g = _grad_out(mod, seed=3)
    ref = _conv_ref(torch.zeros(N_C, c1, *SP_C), w, b, pad, g)[0]
    got = mod._dgrad(g.to(DEV))
    assert got.shape == ref.shape
    assert (got.cpu().double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


@pytest.mark.parametrize("alpha", (0.5, 2.0))
@pytest.mark.parametrize("case", list(CONV_CASES))
def test_quant_conv_backward_matches_fp64_autograd(ops, case, alpha):
    """_QuantConvFn.backward (input gradient of the conv, then the quantiser's backward) against fp64 autograd through
    the five-operation quantiser and F.conv3d.  gx: 1e-5 * max |ref|.  galpha: the bound of A.2 plus
    1e-5 * max |gq_ref| * sum |r - m u|, the conv's error bound carried through the sum."""
    c1, c2, k, pad = CONV_CASES[case]
    levels = 4
    mod, w, b = _module(c1, c2, k, pad, seed=len(case) + 1, levels=levels, alpha=alpha)
    x = _act_input((N_C, c1, *SP_C), alpha, levels, seed=11)
    g = _grad_out(mod, seed=4)
    gx_ref, ga_ref, _, bound = _conv_ref(x, w, b, pad, g, alpha, levels)
    xd = x.to(DEV).requires_grad_(True)
    out = mod(xd)
    assert out.grad_fn is not None
    fwd_ref = F.conv3d(_quant64(x.double(), alpha, levels), w, b, 1, pad)
    assert (out.detach().cpu().double() - fwd_ref).abs().max().item() <= 1e-5 * fwd_ref.abs().max().item()
    gx, ga = torch.autograd.grad(out, [xd, mod.alpha_act], g.to(DEV))
    assert (gx.cpu().double() - gx_ref).abs().max().item() <= 1e-5 * gx_ref.abs().max().item()
    assert ga.shape == mod.alpha_act.shape and ga.dtype == mod.alpha_act.dtype
    assert abs(ga.item() - ga_ref) <= bound, (ga.item(), ga_ref, bound)


def test_quant_conv_backward_first_conv_skips_the_input_gradient(ops):
    """4 -> 32, k = 3, on an input that needs no gradient: None for x, the right galpha."""
    levels, alpha = 16, 2.0
    mod, w, b = _module(4, 32, 3, 1, seed=21, levels=levels, alpha=alpha)
    x = _act_input((N_C, 4, *SP_C), alpha, levels, seed=12)
    g = _grad_out(mod, seed=5)
    _, ga_ref, _, bound = _conv_ref(x, w, b, 1, g, alpha, levels)
    xd = x.to(DEV)
    out = mod(xd)
    (ga,) = torch.autograd.grad(out, [mod.alpha_act], g.to(DEV))
    assert abs(ga.item() - ga_ref) <= bound, (ga.item(), ga_ref, bound)
    # the function itself, asked for alpha only
    from types import SimpleNamespace
    from efficientq_amd.qconv import _QuantConvFn
    ctx = SimpleNamespace(mod=mod, saved_tensors=(xd, mod.alpha_act.detach()), needs_input_grad=(False, True, False))
    gx2, ga2, none = _QuantConvFn.backward(ctx, g.to(DEV))
    assert gx2 is None and none is None and ga2.item() == ga.item()


def test_quant_conv_backward_without_act_quant(ops):
    """q_act=False: the plain conv gradient for x, no gradient for alpha."""
    mod, w, b = _module(16, 32, 3, 1, seed=22, q_act=False)
    x = torch.randn(N_C, 16, *SP_C, generator=torch.Generator().manual_seed(13))
    g = _grad_out(mod, seed=6)
    ref = _conv_ref(x, w, b, 1, g)[0]
    xd = x.to(DEV).requires_grad_(True)
    gx, ga = torch.autograd.grad(mod(xd), [xd, mod.alpha_act], g.to(DEV), allow_unused=True)
    assert ga is None
    assert (gx.cpu().double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_dgrad_follows_weights_written_through_data(ops):
    """The project writes weights through .data, which bumps no version counter and may keep the address: after
    weight.data.copy_(w2) - and after weight.data = w3 - the gradient is that of the new weights."""
    mod, w1, b = _module(16, 32, 3, 1, seed=23)
    g = _grad_out(mod, seed=7)
    gd = g.to(DEV)
    zeros = torch.zeros(N_C, 16, *SP_C)

    def check(w):
        ref = _conv_ref(zeros, w, b, 1, g)[0]
        assert (mod._dgrad(gd).cpu().double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()

    check(w1)
    gen = torch.Generator().manual_seed(24)
    w2 = torch.randn(w1.shape, generator=gen) / float(np.sqrt(w1[0].numel()))
    mod.weight.data.copy_(w2.to(DEV))
    check(w2.double())
    w3 = torch.randn(w1.shape, generator=gen) / float(np.sqrt(w1[0].numel()))
    mod.weight.data = w3.to(DEV)
    check(w3.double())


@pytest.mark.parametrize("kind", ("padding0_k3", "stride2", "padding2_k3"))
def test_dgrad_refuses_what_it_cannot_compute(ops, kind):
    """The gradient conv reuses the forward's padding, which is right only for 2 p = k - 1 at stride 1: anything else
    raises NotImplementedError, from _dgrad and from a backward through the module, and never returns a gradient."""
    stride, pad, match = dict(padding0_k3=(1, 0, "same"), stride2=(2, 1, "strided"), padding2_k3=(1, 2, "same"))[kind]
    mod, _, _ = _module(16, 32, 3, pad, seed=25, stride=stride)
    xd = torch.randn(N_C, 16, *SP_C, generator=torch.Generator().manual_seed(14)).to(DEV).requires_grad_(True)
    out = mod(xd)
    with pytest.raises(NotImplementedError, match=match):
        mod._dgrad(torch.ones_like(out))
    with pytest.raises(NotImplementedError, match=match):
        out.backward(torch.ones_like(out))
    assert xd.grad is None and mod.alpha_act.grad is None


# =================================================================== D. one step of the driver
D_SEED, D_X, D_W1, D_W2 = 0, 0.05, 0.1, 3.0     # input and weight scales: alphas below 1/8, |g_ref| well above 1e-3


def test_tune_activation_range_one_step(ops):
    """PTQConv 4 -> 32 k3, ReLU, PTQConv 32 -> 3 k1 on an 8^3 volume, tune_activation_range(max_iter=1, need_init=True):
    every alpha_act reads the flat buffer the Adam kernel updated, moved by -lr * sign(g_ref) within lr * 2e-5 (the
    first-step identity of B; g_ref: fp64 autograd of the same two-layer function on the CPU, |g_ref| >= 1e-3 for both
    alphas at this seed), and every parameter's requires_grad is what it was.  The input is scaled so that both alphas
    stay below 1/8: half an ulp of the stored fp32 alpha is then below lr * 1e-5."""
    from efficientq_amd import calibrate as K
    from efficientq_amd.qconv import PTQConv
    from efficientq_amd.tune import tune_activation_range
    levels = 4
    gen = torch.Generator().manual_seed(D_SEED)
    c1 = PTQConv(4, 32, 3, 1, 1, bias=True, q_act=True, qlvl_act=levels)
    c2 = PTQConv(32, 3, 1, 1, 0, bias=True, q_act=True, qlvl_act=levels)
    with torch.no_grad():
        c1.weight.copy_(torch.randn(c1.weight.shape, generator=gen) * D_W1)
        c1.bias.copy_(torch.randn(32, generator=gen) * 0.01)
        c2.weight.copy_(torch.randn(c2.weight.shape, generator=gen) * D_W2)
        c2.bias.copy_(torch.randn(3, generator=gen) * 0.1)
    model = torch.nn.Sequential(c1, torch.nn.ReLU(), c2)
    mods = [c1, c2]
    c1.weight.requires_grad_(False)
    c2.bias.requires_grad_(False)
    x = torch.randn(2, 4, 8, 8, 8, generator=gen) * D_X
    model.to(DEV)
    xd = x.to(DEV)
    K.set_fp(model)
    with torch.no_grad():
        output_fp = model(xd).detach()
    K.set_init_alpha(model)                      # the init pass the call repeats: the alphas the step starts from
    with torch.no_grad():
        model(xd)
    a0 = [m.alpha_act.detach().cpu().item() for m in mods]
    assert all(0 < a < 0.125 for a in a0), a0
    before = [(n, p.requires_grad) for n, p in model.named_parameters()]

    losses = tune_activation_range(model, output_fp, xd, max_iter=1, need_init=True)
    assert len(losses) == 1

    # the same function in fp64 on the CPU
    al = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in a0]
    w1, b1, w2, b2 = (t.detach().cpu().double() for t in (c1.weight, c1.bias, c2.weight, c2.bias))
    h = torch.relu(F.conv3d(_quant64(x.double(), al[0], levels), w1, b1, 1, 1))
    out = F.conv3d(_quant64(h, al[1], levels), w2, b2, 1, 0)
    loss = F.mse_loss(out, output_fp.cpu().double())
    g_ref = [g.item() for g in torch.autograd.grad(loss, al)]
    print(f"tune step: alphas {a0}, g_ref {g_ref}, loss {losses[0]:.6g} (fp64 {loss.item():.6g})")
    assert all(abs(g) >= 1e-3 for g in g_ref), g_ref                     # none skipped at this seed

    a1 = [m.alpha_act.detach().cpu().item() for m in mods]
    for a_old, a_new, g in zip(a0, a1, g_ref):
        assert abs((a_new - a_old) + LR * np.sign(g)) <= LR * 2e-5, (a_old, a_new, g, (a_new - a_old) / LR)
    # one flat buffer behind every alpha_act, element i for module i
    ptr0 = mods[0].alpha_act.data.data_ptr()
    for i, m in enumerate(mods):
        assert m.alpha_act.data.dim() == 0 and m.alpha_act.data.data_ptr() == ptr0 + 4 * i
        assert m.alpha_act.data.untyped_storage().data_ptr() == ptr0
    assert [(n, p.requires_grad) for n, p in model.named_parameters()] == before
