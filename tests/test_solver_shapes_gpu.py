"""Every dispatch class of the prox solver and of the SPD inverse (csrc/prox_solve.hip, csrc/spd_inverse.hip) against fp64 (-m gpu).

effq_prox_solve* picks one of six GEMM variants plus a K split from (c2, n), effq_spd_inverse the rank-64 or the 256-row
sweep from n.  Each case here first asserts, through effq_prox_plan_query / effq_spd_inverse_plan, the class it was chosen
for - a retuned threshold then fails the case instead of silently moving it to a class that is tested elsewhere - and then
compares the kernels with fp64 arithmetic on the same inputs:

  a. the product W* = Bm * A^-1 on every variant: the shapes of the 1x1x1 transition layers of the shipped networks
     (n = 64 k + 1: the bias column alone in the last column tile), row remainders, both sides of the bf16 switch, systems
     without padding and without bias, K splits that do not divide the K tiles, the scalar build / reduce kernels;
  b. effq_prox_solve_shifted with its ~26 terms on variants 0, 1 and the split variant 2;
  c. the inverse at one block, exact multiples of 64, the switch to the wide sweep (99 -> 100 blocks) and last pivot blocks
     of 1, 2, 3 and 4 64-blocks;
  d. effq_admm_run (projection writes the next right-hand side into Bm, the solve runs on the padding and the bias column an
     earlier build left) against the same iterations issued one public op at a time: equal bits.

Outputs land between guard bands and in NaN-filled blocks, and every case runs a second time on a workspace filled with
0xFF bytes (NaN as floats and as doubles): the library zero-fills a workspace only when it allocates it, and a calibration
reuses it layer after layer with other paddings."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                     # floats on either side of an output (keeps the output 256-byte aligned)
SENTINEL = -7.25e33
PROX_KT = {0: 32, 1: 32, 2: 32, 3: 32, 5: 16, 7: 16}     # K tile of each variant (PBK / B3_K of prox_solve.hip)


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_ops(DEV)


def dev(t):
    return None if t is None else t.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(*shape):
    """A NaN-filled device tensor of `shape` inside a larger sentinel-filled buffer: (buffer, view)."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + numel].view(*shape)
    view.fill_(float("nan"))
    return buf, view


def _guards_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all().item()) and bool((buf[-GUARD:] == SENTINEL).all().item())


# ------------------------------------------------------------------ a. the product, every class
# n, c2, bias, variant, gy, split, why
PROX_CASES = [
    # the shipped networks' layers that no kernel test reached (n = c1 k^3 + 1)
    (129, 256, True, 0, 1, False, "BraTS down 128->256, 1^3"),
    (257, 512, True, 0, 2, False, "LiTS down 256->512, 1^3: two row tiles"),
    (513, 256, True, 0, 1, True, "LiTS up 512->256, 1^3: the fill-search split, 17 K tiles in 2 slices"),
    (65, 128, True, 1, 1, False, "64->128, 1^3"),
    (257, 128, True, 1, 1, False, "256->128, 1^3"),
    (1729, 64, True, 2, 1, True, "64->64, 3^3: 55 K tiles in 9 slices"),
    (33, 64, True, 2, 1, False, "32->64, 1^3"),
    (109, 32, True, 3, 1, False, "4->32, 3^3"),
    (33, 3, True, 3, 1, False, "classifier"),
    # row remainders on each f32 variant
    (513, 200, True, 0, 1, True, "variant 0, one ragged row tile"),
    (513, 300, True, 0, 2, True, "variant 0, second row tile ragged"),
    (257, 100, True, 1, 1, False, "variant 1, ragged rows"),
    (130, 40, True, 2, 1, False, "variant 2, ragged rows"),
    (130, 3, True, 3, 1, False, "variant 3, ragged rows"),
    # the two sides of the bf16 switch (n = 1024); 1023: scalar build AND scalar reduce, 32 K tiles in 5 slices
    (1023, 128, True, 1, 1, True, "last f32 size at 128 rows"),
    (1024, 128, True, 7, 1, True, "first bf16x3 size at 128 rows"),
    (1023, 256, True, 0, 1, True, "last f32 size at 256 rows"),
    (1024, 256, True, 5, 1, True, "first bf16x3 size at 256 rows"),
    (1729, 256, True, 5, 1, True, "variant 5: 110 K tiles in 6 slices"),
    # no padding (ldb == lda == n) and no bias (b0 = bstar = NULL): the --blk pre layers, n = 27 c1
    (864, 32, False, 3, 1, True, "32->32 3^3 without bias"),
    (1728, 64, False, 2, 1, True, "64->64 3^3 without bias"),
    (3456, 128, False, 7, 1, True, "128->128 3^3 without bias"),
    (128, 256, False, 0, 1, False, "128->256 1^3 without bias"),
    (256, 128, False, 1, 1, False, "256->128 1^3 without bias"),
    # (n - bias) % 4 != 0: the scalar build kernel (and, split, the scalar reduce) on variants 0 and 1
    (131, 256, True, 0, 1, False, "scalar build, variant 0"),
    (259, 128, True, 1, 1, False, "scalar build, variant 1"),
    (515, 256, True, 0, 1, True, "scalar build and reduce, variant 0"),
]
# K splits whose slice count does not divide the K-tile count (uneven slices), on variants 0, 2 and 5 (and 1)
UNEVEN_SPLITS = {(513, 256), (1729, 64), (1729, 256), (1023, 128), (1023, 256)}
_prox_worst = {}


def _prox_operands(n, c2, bias, seed):
    gen = torch.Generator().manual_seed(seed)
    nw = n - int(bias)
    B0 = torch.randn(c2, n, generator=gen) * 10
    W0 = torch.randn(c2, nw, generator=gen)
    b0 = torch.randn(c2, generator=gen) if bias else None
    G = torch.randn(c2, nw, generator=gen)
    dual = torch.randn(c2, nw, generator=gen) * 0.1
    return B0, W0, b0, G, dual


def _build_bm_fp32(B0, W0, b0, G, dual, rho, eta):
    """Bm exactly as the build kernels form it in fp32 (solver.py:316-322 op order)."""
    nw = W0.shape[1]
    Bm = (B0[:, :nw] + np.float32(eta) * W0) + np.float32(rho) * (G - dual)
    if b0 is not None:
        Bm = torch.cat([Bm, (B0[:, -1] + np.float32(eta) * b0)[:, None]], 1)
    return Bm


@pytest.mark.parametrize("n,c2,bias,variant,gy,split,why", PROX_CASES,
                         ids=[f"n{c[0]}-c{c[1]}-{'bias' if c[2] else 'nobias'}" for c in PROX_CASES])
def test_prox_product_in_every_dispatch_class(ops, n, c2, bias, variant, gy, split, why):
    """What = Bm * Ainv against the fp64 product of the SAME fp32 operands, construction and acceptance of
    test_prox_product_is_fp32_grade_on_every_kernel_variant: |got - want| <= 4e-7 (|Bm| |S|) element-wise and
    max |got - want| <= 2e-6 max |want|."""
    plan = ops.prox_plan(c2, n)
    assert (plan["variant"], plan["gy"], plan["nsplit"] > 1) == (variant, gy, split), (why, plan)
    nkt = ops.lib.effq_ainv_ld(n) // PROX_KT[variant]
    if (n, c2) in UNEVEN_SPLITS:
        assert plan["nsplit"] > 1 and nkt % plan["nsplit"] != 0, (nkt, plan)
    nw = n - int(bias)
    lda = ops.lib.effq_ainv_ld(n)
    gen = torch.Generator().manual_seed(7 * n + c2)
    S = torch.randn(n, n, generator=gen) * 1e-3
    S = 0.5 * (S + S.T)                                            # the kernels use the symmetry of A^-1
    Ainv = torch.zeros(n, lda)
    Ainv[:, :n] = S
    B0, W0, b0, G, dual = _prox_operands(n, c2, bias, n + c2)
    rho, eta = 30.0, 3.0
    dB0, dA, dW0, db0, dG, ddual = dev(B0), dev(Ainv), dev(W0), dev(b0), dev(G), dev(dual)

    def run():
        wbuf, wstar = _guarded(c2, nw)
        bbuf, bstar = _guarded(c2) if bias else (None, None)
        ops.prox_solve(dB0, dA, dW0, db0, dG, ddual, rho, eta, wstar, bstar)
        torch.cuda.synchronize()
        assert _guards_untouched(wbuf), "prox_solve wrote outside wstar"
        assert bbuf is None or _guards_untouched(bbuf), "prox_solve wrote outside bstar"
        return wstar, bstar

    wstar, bstar = run()
    Bm = _build_bm_fp32(B0, W0, b0, G, dual, rho, eta)
    want = Bm.double() @ S.double()
    bound = Bm.double().abs() @ S.double().abs()
    got = (torch.cat([wstar.cpu(), bstar.cpu()[:, None]], 1) if bias else wstar.cpu()).double()
    err = (got - want).abs()
    frac = (max((err / (4e-7 * bound)).max().item(), err.max().item() / (2e-6 * want.abs().max().item()))
            if torch.isfinite(got).all() else float("inf"))
    _prox_worst[(n, c2)] = frac
    print(f"prox n={n} c2={c2} {plan}: error / bound = {frac:.3f} (worst so far {max(_prox_worst.values()):.3f})")
    assert (err <= 4e-7 * bound).all(), (err / bound).max()
    assert err.max() <= 2e-6 * want.abs().max()
    # the same call on a dirty workspace: Bm's zero padding and the K slices must be rewritten by the kernels themselves
    ops._ws["prox"].fill_(0xFF)
    wstar2, bstar2 = run()
    assert torch.equal(_bits(wstar2), _bits(wstar))
    assert bstar is None or torch.equal(_bits(bstar2), _bits(bstar))


# ------------------------------------------------------------------ b. the shifted solve
def _conditioned_system(n, bias, seed, rho=30.0, eta=3.0):
    """A0 = 2 X X^T (X: n x 3n) and the fp64 system matrix A = A0 + rho I' + eta I (test_spd_inverse_and_prox)."""
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(n, 3 * n, generator=gen)
    A0 = (2 * X @ X.T).float()
    d = torch.full((n,), rho + eta, dtype=torch.float64)
    if bias:
        d[-1] = eta
    return A0, A0.double() + torch.diag(d), gen


_shift_worst = {}


@pytest.mark.parametrize("n,c2,variant,split", [(129, 256, 0, False), (257, 128, 1, False), (1729, 64, 2, True)])
def test_shifted_prox_solve_on_the_transition_layer_shapes(ops, n, c2, variant, split):
    """effq_prox_solve_shifted (term > 0 feeds wstar back through the build kernels) against the direct fp64 solve of the
    rho / 2 system, as the tail of test_spd_inverse_and_prox: max |got - want| <= 3e-5 max |want|."""
    plan = ops.prox_plan(c2, n)
    assert (plan["variant"], plan["nsplit"] > 1) == (variant, split), plan
    rho, eta = 30.0, 3.0
    A0, A, gen = _conditioned_system(n, True, n, rho, eta)
    Ainv = ops.spd_inverse(dev(A0), True, rho, eta)
    B0 = torch.randn(c2, n, generator=gen) * 10
    W0 = torch.randn(c2, n - 1, generator=gen)
    b0 = torch.randn(c2, generator=gen)
    G = torch.randn(c2, n - 1, generator=gen)
    dual = torch.randn(c2, n - 1, generator=gen) * 0.1
    rho0 = rho / 2
    assert ops.shift_terms(rho0, eta, rho) > 2
    A_half = A - torch.diag(torch.cat([torch.full((n - 1,), rho - rho0, dtype=torch.float64),
                                       torch.zeros(1, dtype=torch.float64)]))
    Bm0 = B0.double() + eta * torch.cat([W0, b0[:, None]], 1).double()
    Bm0[:, :-1] += rho0 * (G - dual).double()
    want0 = torch.linalg.solve(A_half, Bm0.T).T
    dB0, dW0, db0, dG, ddual = dev(B0), dev(W0), dev(b0), dev(G), dev(dual)

    def run():
        wbuf, wstar = _guarded(c2, n - 1)
        bbuf, bstar = _guarded(c2)
        ops.prox_solve_shifted(dB0, Ainv, dW0, db0, dG, ddual, rho0, eta, rho, wstar, bstar)
        torch.cuda.synchronize()
        assert _guards_untouched(wbuf) and _guards_untouched(bbuf)
        return wstar, bstar

    wstar, bstar = run()
    got0 = torch.cat([wstar.cpu(), bstar.cpu()[:, None]], 1).double()
    err = (got0 - want0).abs().max().item()
    _shift_worst[n] = err / (3e-5 * want0.abs().max().item())
    print(f"shifted n={n} c2={c2}: error / bound = {_shift_worst[n]:.3f}")
    assert err <= 3e-5 * want0.abs().max()
    ops._ws["prox"].fill_(0xFF)
    wstar2, bstar2 = run()
    assert torch.equal(_bits(wstar2), _bits(wstar)) and torch.equal(_bits(bstar2), _bits(bstar))


# ------------------------------------------------------------------ c. the inverse, every class
def _fresh_inverse_workspace(ops):
    """Drop the inverse workspace: the next spd_inverse allocates a zero-filled one of exactly its own size."""
    torch.cuda.synchronize()
    old = ops._ws.pop("inv", None)
    if old is not None:
        ops._ws_retired.append(old)


# n, bias, wide, nblk
INV_SMALL = [(1, True, False, 1), (63, True, False, 1), (64, True, False, 1), (65, True, False, 2),
             (128, True, False, 2), (129, True, False, 3), (257, True, False, 5), (513, True, False, 9),
             (64, False, False, 1), (128, False, False, 2), (864, False, False, 14)]


@pytest.mark.parametrize("n,bias,wide,nblk", INV_SMALL,
                         ids=[f"n{c[0]}-{'bias' if c[1] else 'nobias'}" for c in INV_SMALL])
def test_spd_inverse_small_sizes_against_lapack(ops, n, bias, wide, nblk):
    """One block, exact multiples of 64 (no identity padding) and the 1x1x1 sizes against torch.linalg.inv in fp64, recipe
    and bound of test_spd_inverse_and_prox: max |Ainv - want| <= 2e-7 max |want| + 1e-12."""
    plan = ops.spd_inverse_plan(n)
    assert (plan["wide"], plan["nblk"]) == (wide, nblk), plan
    rho, eta = 30.0, 3.0
    A0, A, _ = _conditioned_system(n, bias, 1000 + n, rho, eta)
    want = torch.linalg.inv(A)
    dA0 = dev(A0)
    Ainv_pad = ops.spd_inverse(dA0, bias, rho, eta)
    assert Ainv_pad.shape == (n, ops.lib.effq_ainv_ld(n)) and Ainv_pad.shape[1] % 32 == 0
    assert Ainv_pad[:, n:].abs().sum().item() == 0
    err = (Ainv_pad.cpu()[:, :n].double() - want).abs().max().item()
    print(f"inverse n={n} {plan}: error / bound = {err / (2e-7 * want.abs().max().item() + 1e-12):.3f}")
    assert err <= 2e-7 * want.abs().max() + 1e-12
    assert torch.equal(Ainv_pad[:, :n], Ainv_pad[:, :n].T)
    torch.cuda.synchronize()
    ops._ws["inv"].fill_(0xFF)                       # the identity padding of A64 is the kernels' to write
    again = ops.spd_inverse(dA0, bias, rho, eta)
    assert torch.equal(_bits(again), _bits(Ainv_pad))


def _large_system(n, bias):
    """A0 of test_solver_at_the_largest_system_sizes: 2 X X^T with X n x 2n on the device, a bias row of ones."""
    gen = torch.Generator(device=DEV).manual_seed(n)
    X = torch.randn(n, 2 * n, device=DEV, generator=gen)
    if bias:
        X[-1] = 1.0
    A0 = (2.0 * (X @ X.T)).contiguous()
    del X
    return A0, 10.0 * n, 1.0 * n


def _inverse_residual(A0, Ainv, n, bias, rho, eta):
    d = torch.full((n,), rho + eta, dtype=torch.float64, device=DEV)
    if bias:
        d[-1] = eta
    A64 = A0.double() + torch.diag(d)
    X64 = Ainv[:, :n].double()
    R = A64 @ X64
    R.diagonal().sub_(1.0)
    return (R.norm() / (A64.norm() * X64.norm())).item()


# n, bias, wide, nblk, 64-blocks of the last pivot block
INV_LARGE = [(1728, False, False, 27, 1), (1729, True, False, 28, 1),
             (6336, True, False, 99, 1),       # the last rank-64 size
             (6337, True, True, 100, 4),       # the first wide size: 63 padded rows
             (6400, False, True, 100, 4),      # no padding, no bias
             (6401, True, True, 101, 1), (6500, True, True, 102, 2), (6592, True, True, 103, 3)]


@pytest.mark.parametrize("n,bias,wide,nblk,last", INV_LARGE,
                         ids=[f"n{c[0]}-{'bias' if c[1] else 'nobias'}" for c in INV_LARGE])
def test_spd_inverse_around_the_wide_sweep_switch(ops, n, bias, wide, nblk, last):
    """The device-side fp64 residual of test_solver_at_the_largest_system_sizes with its recipe and bounds:
    |A X - I|_F / (|A|_F |X|_F) <= 1e-7 and X exactly symmetric; zero padding columns."""
    plan = ops.spd_inverse_plan(n)
    assert (plan["wide"], plan["nblk"]) == (wide, nblk), plan
    if wide:
        assert plan["pivot_blocks"] == (nblk + 3) // 4 and nblk - 4 * (plan["pivot_blocks"] - 1) == last, plan
    else:
        assert plan["pivot_blocks"] == nblk
    A0, rho, eta = _large_system(n, bias)
    Ainv = ops.spd_inverse(A0, bias, rho, eta)
    assert Ainv.shape == (n, ops.lib.effq_ainv_ld(n))
    assert Ainv[:, n:].abs().sum().item() == 0
    assert torch.equal(Ainv[:, :n], Ainv[:, :n].T)
    res = _inverse_residual(A0, Ainv, n, bias, rho, eta)
    print(f"inverse n={n} {plan}: residual / bound = {res / 1e-7:.3f}")
    assert res <= 1e-7
    torch.cuda.synchronize()
    ops._ws["inv"].fill_(0xFF)
    again = ops.spd_inverse(A0, bias, rho, eta)
    assert torch.equal(_bits(again), _bits(Ainv))


def test_spd_inverse_in_a_workspace_that_held_a_larger_sweep(ops):
    """n = 6401 (101 blocks) right after n = 6592 (103 blocks) in the same workspace, and after a 0xFF fill: the bits of its
    first run, made in a freshly allocated (zero-filled) workspace of its own size."""
    _fresh_inverse_workspace(ops)
    A0, rho, eta = _large_system(6401, True)
    first = ops.spd_inverse(A0, True, rho, eta)
    assert _inverse_residual(A0, first, 6401, True, rho, eta) <= 1e-7
    Abig, rho_b, eta_b = _large_system(6592, True)
    big = ops.spd_inverse(Abig, True, rho_b, eta_b)
    assert _inverse_residual(Abig, big, 6592, True, rho_b, eta_b) <= 1e-7
    del Abig, big
    assert ops._ws["inv"].numel() >= ops.lib.effq_spd_inverse_ws_bytes(6592)
    after_larger = ops.spd_inverse(A0, True, rho, eta)
    assert torch.equal(_bits(after_larger), _bits(first))
    torch.cuda.synchronize()
    ops._ws["inv"].fill_(0xFF)
    after_fill = ops.spd_inverse(A0, True, rho, eta)
    assert torch.equal(_bits(after_fill), _bits(first))


# ------------------------------------------------------------------ d. one layer through effq_admm_run
def _rho_schedule(rho, rho_max, iters, period):
    """(rho of iteration i, the dual's divisor after it) of EfficientQConv.py:129-137."""
    out = []
    for i in range(iters):
        div = 1.0
        nxt = rho
        if i % period == 0:
            div = 2.0 if rho * 2 <= rho_max else rho_max / rho
            nxt = rho * 2 if rho * 2 <= rho_max else rho_max
        out.append((rho, div))
        rho = nxt
    return out


@pytest.mark.parametrize("c1,c2,variant", [(128, 256, 0), (256, 128, 1)])
def test_fused_admm_iterates_equal_the_step_by_step_ops(ops, c1, c2, variant):
    """effq_admm_run on a 1x1x1 transition layer against the same iterations from prox_solve[_shifted], the weight fixed
    point and admm_project_dual.  From the second iteration on the fused run solves on a Bm whose weight columns the
    projection wrote (effq_project_dual_next) and whose bias column and padding the first build left; the build arithmetic
    is the same fp32 op order, so every iterate in G_ring / b_ring, every scale and the final dual must be EQUAL.

    The step-by-step loop takes the fixed point the run takes for 32768 weights at 4 levels, the bucketed one
    (fixed_point_bucket; admm_plan: 4096 < nw <= 2^19, <= 16 levels).  With the all-values kernel (weight_fixed_point)
    instead, the first difference is the weight scale of iteration 2 (128 -> 256: 0.14919563380180575 against
    0.14919563380180567, 5e-16 relative; every earlier iterate, scale and solve equal): effq_hip.h documents that pair as
    "alpha agrees to ~1e-14 relative (fp64 sums in another order), same iteration count", and that is what is asserted of
    it here, per iteration, on the same input - the only step that may round differently, and it is not part of the
    compared chain."""
    from efficientq_amd.hip_ops import make_geom, to_ndhwc
    n = c1 + 1
    plan = ops.prox_plan(c2, n)
    assert (plan["variant"], plan["nsplit"]) == (variant, 1), plan
    gen = torch.Generator().manual_seed(c1 + 3 * c2)
    x = torch.relu(torch.randn(2, c1, 6, 6, 8, generator=gen))
    w = torch.randn(c2, c1, 1, 1, 1, generator=gen) * 0.1
    b = torch.randn(c2, generator=gen) * 0.1
    y = F.conv3d(x, w, b)
    geom = make_geom(x.shape, c2, 1, 1, 0)
    xq, yn = dev(to_ndhwc(x)), dev(to_ndhwc(y))
    W0, b0 = dev(w.reshape(c2, c1).contiguous()), dev(b)
    A0, B0 = ops.gram(xq, None, yn, geom, True)
    # EfficientQConv.py:43-49: rho, rho_max, eta = (10, 1000, 1) * scale; rho_max cut so that the schedule also takes its
    # capped step (dual divided by rho_max / rho) inside a handful of iterations
    scale = max(y.numel() * y.std().item() / (w.numel() * w.std().item()), 1.0)
    rho, rho_max, eta = 10.0 * scale, 50.0 * scale, 1.0 * scale
    iters, period, levels = 7, 2, 4
    sched = _rho_schedule(rho, rho_max, iters, period)
    assert [d for _, d in sched] == pytest.approx([2.0, 1.0, 2.0, 1.0, 1.25, 1.0, 1.0])
    n_inv = ops.lib.effq_admm_num_inverses(rho, rho_max, iters, period)
    distinct = sorted({r for r, _ in sched})
    assert n_inv == len(distinct) - 1            # iteration 0 alone has the first rho: solved through the second's inverse

    run = ops.admm_run(A0, B0, W0, b0, geom, yn, xq=xq, rho=rho, rho_max=rho_max, eta=eta, iters=iters, period=period,
                       levels=levels, channel_wise=False)
    torch.cuda.synchronize()
    assert int(run.err.item()) == 0

    G = W0.clone()
    dual = torch.zeros_like(W0)
    wstar, v = torch.empty_like(W0), torch.empty_like(W0)
    bstar = torch.empty(c2, device=DEV)
    st, st_all, v_all = ops.new_fp_state(), ops.new_fp_state(), torch.empty_like(W0)
    assert 4096 < W0.numel() <= ops.lib.effq_fp_small_max() and not ops.lib.effq_admm_uses_traj(W0.numel(), levels)
    inverses = {}
    for i, (rho_i, div) in enumerate(sched):
        rho_use = sched[1][0] if i == 0 else rho_i
        if rho_use not in inverses:
            inverses[rho_use] = ops.spd_inverse(A0, True, rho_use, eta)
        if i == 0:
            ops.prox_solve_shifted(B0, inverses[rho_use], W0, b0, G, dual, rho_i, eta, rho_use, wstar, bstar)
        else:
            ops.prox_solve(B0, inverses[rho_use], W0, b0, G, dual, rho_i, eta, wstar, bstar)
        ops.fixed_point_bucket(wstar.view(-1), dual.view(-1), v.view(-1), levels, st)
        ops.weight_fixed_point(wstar.view(-1), dual.view(-1), v_all.view(-1), levels, st_all)
        Gn = torch.empty_like(W0)
        ops.admm_project_dual(v.view(-1), wstar.view(-1), st, levels, Gn.view(-1), dual.view(-1), div)
        torch.cuda.synchronize()
        where = f"iteration {i} (rho {rho_i:g}, dual divisor {div:g})"
        assert torch.equal(_bits(run.b_ring[i]), _bits(bstar)), \
            f"{where}: prox solve, bias column differs by {(run.b_ring[i] - bstar).abs().max().item():.3e}"
        assert run.state_ring[i, 0].item() == st[0].item(), \
            f"{where}: weight scale {run.state_ring[i, 0].item()!r} != {st[0].item()!r}"
        (a_all, it_all, _), (a_bkt, it_bkt, _) = ops.read_fp_state(st_all), ops.read_fp_state(st)
        assert torch.equal(_bits(v_all), _bits(v)) and it_all == it_bkt and abs(a_all - a_bkt) <= 1e-14 * abs(a_bkt), \
            f"{where}: all-values fixed point {a_all!r} in {it_all} iterations, bucketed {a_bkt!r} in {it_bkt}"
        diff = (run.G_ring[i].view_as(Gn) - Gn).abs().max().item()
        assert torch.equal(_bits(run.G_ring[i]), _bits(Gn.view(-1))), f"{where}: projected weights differ by {diff:.3e}"
        G = Gn
    assert torch.equal(_bits(run.wstar), _bits(wstar.view(-1))), "last prox solve, weight columns"
    assert torch.equal(_bits(run.dual), _bits(dual.view(-1))), "final dual"
    assert len(inverses) == n_inv


@pytest.mark.parametrize("c1,c2,k,shape,fused", [(32, 32, 1, (2, 32, 4, 4, 8), True), (1, 8, 3, (2, 1, 6, 6, 8), False)],
                         ids=["small-kernel-epilogue", "scalar-projection-next-rhs"])
def test_fused_admm_projection_paths_equal_the_step_by_step_ops(ops, c1, c2, k, shape, fused):
    """The construction, schedule and equalities of test_fused_admm_iterates_equal_the_step_by_step_ops on the two ways
    through the projection that its layers do not take; both layers have nw <= 4096, where effq_admm_run takes the
    single-workgroup all-values fixed point, and the step-by-step loop takes the same kernel (weight_fixed_point).

    small-kernel-epilogue: rows of 32 weights and 16-byte aligned ring slots - the run does the projection, the dual update
    and the next right-hand side inside the fixed-point kernel; the loop with the stand-alone vector kernel.
    scalar-projection-next-rhs: rows of 27 weights - nothing is fused, the run's projection is the element-by-element kernel
    (level index from the fp64 arithmetic) and writes Bm one float at a time; the loop's is the vector kernel on 216 aligned
    weights (level index from the fp32 screen)."""
    from efficientq_amd.hip_ops import make_geom, to_ndhwc
    nwrow = c1 * k ** 3
    nw = c2 * nwrow
    assert nw <= 4096 and nw % 4 == 0 and (nwrow % 4 == 0) == fused
    gen = torch.Generator().manual_seed(c1 + 3 * c2)
    x = torch.relu(torch.randn(*shape, generator=gen))
    w = torch.randn(c2, c1, k, k, k, generator=gen) * 0.1
    b = torch.randn(c2, generator=gen) * 0.1
    y = F.conv3d(x, w, b, padding=k // 2)
    geom = make_geom(x.shape, c2, k, 1, k // 2)
    xq, yn = dev(to_ndhwc(x)), dev(to_ndhwc(y))
    W0, b0 = dev(w.reshape(c2, nwrow).contiguous()), dev(b)       # (c1 = 1 or k = 1: every row order is this one)
    A0, B0 = ops.gram(xq, None, yn, geom, True)
    scale = max(y.numel() * y.std().item() / (w.numel() * w.std().item()), 1.0)
    rho, rho_max, eta = 10.0 * scale, 50.0 * scale, 1.0 * scale
    iters, period, levels = 7, 2, 4
    sched = _rho_schedule(rho, rho_max, iters, period)
    assert [d for _, d in sched] == pytest.approx([2.0, 1.0, 2.0, 1.0, 1.25, 1.0, 1.0])
    n_inv = ops.lib.effq_admm_num_inverses(rho, rho_max, iters, period)
    assert n_inv == len({r for r, _ in sched}) - 1

    run = ops.admm_run(A0, B0, W0, b0, geom, yn, xq=xq, rho=rho, rho_max=rho_max, eta=eta, iters=iters, period=period,
                       levels=levels, channel_wise=False)
    torch.cuda.synchronize()
    assert int(run.err.item()) == 0
    assert run.G_ring.data_ptr() % 16 == 0 and run.v.data_ptr() % 16 == 0 and run.dual.data_ptr() % 16 == 0

    G = W0.clone()
    dual = torch.zeros_like(W0)
    wstar, v = torch.empty_like(W0), torch.empty_like(W0)
    bstar = torch.empty(c2, device=DEV)
    st = ops.new_fp_state()
    inverses = {}
    for i, (rho_i, div) in enumerate(sched):
        rho_use = sched[1][0] if i == 0 else rho_i
        if rho_use not in inverses:
            inverses[rho_use] = ops.spd_inverse(A0, True, rho_use, eta)
        if i == 0:
            ops.prox_solve_shifted(B0, inverses[rho_use], W0, b0, G, dual, rho_i, eta, rho_use, wstar, bstar)
        else:
            ops.prox_solve(B0, inverses[rho_use], W0, b0, G, dual, rho_i, eta, wstar, bstar)
        ops.weight_fixed_point(wstar.view(-1), dual.view(-1), v.view(-1), levels, st)
        Gn = torch.empty_like(W0)
        ops.admm_project_dual(v.view(-1), wstar.view(-1), st, levels, Gn.view(-1), dual.view(-1), div)
        torch.cuda.synchronize()
        where = f"iteration {i} (rho {rho_i:g}, dual divisor {div:g})"
        assert torch.equal(_bits(run.b_ring[i]), _bits(bstar)), \
            f"{where}: prox solve, bias column differs by {(run.b_ring[i] - bstar).abs().max().item():.3e}"
        assert run.state_ring[i, 0].item() == st[0].item(), \
            f"{where}: weight scale {run.state_ring[i, 0].item()!r} != {st[0].item()!r}"
        diff = (run.G_ring[i].view_as(Gn) - Gn).abs().max().item()
        assert torch.equal(_bits(run.G_ring[i]), _bits(Gn.view(-1))), f"{where}: projected weights differ by {diff:.3e}"
        G = Gn
    assert torch.equal(_bits(run.wstar), _bits(wstar.view(-1))), "last prox solve, weight columns"
    assert torch.equal(_bits(run.dual), _bits(dual.view(-1))), "final dual"
    assert len(inverses) == n_inv
