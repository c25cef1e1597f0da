"""The paths of effq_admm_run (csrc/admm_run.hip) that carry the wide layers, iteration by iteration (-m gpu).

tests/test_solver_shapes_gpu.py (section d) proves "fused run == the same iterations one public op at a time" for the bucketed
and the small fixed point, on 7 iterations that can never reach the trajectory kernel, and never looks at `hist`.  Here:

  a. the same equality over 34 iterations at period 16 (rho changes after iterations 0, 16 and 32; the trajectory kernel runs at
     13-16 and 29-32 and hands back to the older kernel at 33) on the remaining classes of fp_kind(): traj fed by a whole
     product, traj fed by K slices (effq_prox_enqueue with parts + effq_fixed_point_traj_parts), traj warmed by the
     cooperative recorder, coop alone, and the channel kernel against its own public op - with an oracle / fp64 anchor on the
     trajectory iterations and on the first iteration after every change of rho, and hist of all 34 slots against conv_step
     (nine hand-overs to the loss stream on its four recycled events);
  b. hist[j] is the loss of iterate j: every ring slot re-evaluated by the stand-alone entry point of each loss kind, with and
     without the loss stream, on 11 iterations at period 4 (conv groups 4 + 4 + 3, Gram groups 8 + 3);
  c. effq_admm_select_best against the reference's `if i == 0 or loss < best` on hand-built histories and rings;
  d. k_admm_residuals above its single-pass span (inside a.), effq_gram_pack / effq_gram_unpack above their grid.

Every case first asserts the dispatch class it was built for, from the library's own queries and the rules of admm_plan /
fp_kind restated here: a retuned threshold then fails the case instead of silently moving it to another class."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import effq_oracle as O
from tests.projection_ref import ref_project
from tests.test_solver_shapes_gpu import _rho_schedule

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U53 = 2.0 ** -53
TAG = "[admm-run-paths]"


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    handle = get_ops(DEV)
    found = dict(handle._ws)
    yield handle
    # Leave the shared handle and the caching allocator as they were found.  This module is the first of the suite by name
    # and frees blocks of many sizes (rings of 34 iterates, 560 000-weight tensors); tests/test_conv_tiles_gpu.py::_poison
    # relies on the allocator handing the NaN-filled block it has just freed to the next allocation of that size, and
    # an equal block that this module left cached at a lower address is handed out instead.  So: the workspaces this module
    # made the handle grow are dropped, and every cached block goes back to the driver.
    torch.cuda.synchronize()
    handle._ws = found
    handle.release_retired()
    torch.cuda.empty_cache()


def dev(t):
    return None if t is None else t.to(DEV)


def _bits(t):
    """The bit pattern of an fp32 / fp64 tensor or array (NaNs and signed zeros compare as what they are)."""
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t).view(np.int32 if t.dtype == np.float32 else np.int64)
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    return torch.equal(_bits(a).reshape(-1), _bits(b).reshape(-1))


def _layer(c1, c2, k, seed):
    """The construction of test_fused_admm_iterates_equal_the_step_by_step_ops: a ReLU input of 2 x c1 x 6 x 6 x 8, the FP
    conv's output as the target, rho / rho_max / eta = (10, 50, 1) x the reference's scale (EfficientQConv.py:43-49)."""
    from efficientq_amd.hip_ops import make_geom
    gen = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(2, c1, 6, 6, 8, generator=gen))
    w = torch.randn(c2, c1, k, k, k, generator=gen) * 0.1
    b = torch.randn(c2, generator=gen) * 0.1
    y = F.conv3d(x, w, b, padding=k // 2)
    scale = max(y.numel() * y.std().item() / (w.numel() * w.std().item()), 1.0)
    return SimpleNamespace(x=x, w=w, b=b, y=y, geom=make_geom(x.shape, c2, k, 1, k // 2), pad=k // 2,
                           rho=10.0 * scale, rho_max=50.0 * scale, eta=1.0 * scale)


# ------------------------------------------------------------------ a. fused run == step-by-step ops: traj, coop, channels
ITERS, PERIOD = 34, 16
TRAJ_ITERS = [13, 14, 15, 16, 29, 30, 31, 32]
# id: (c1, c2, k, weight levels, channel mode, classes the iterations must take, prox K split, residuals)
RUN_CASES = {
    "traj-whole": (256, 256, 1, 4, False, {"traj", "bucket"}, False, False),
    "traj-parts": (64, 64, 3, 4, False, {"traj", "bucket"}, True, False),
    "coop-records-traj": (144, 144, 3, 4, False, {"traj", "coop"}, True, True),
    "coop": (256, 160, 1, 32, False, {"coop"}, False, False),
    "channels": (64, 64, 3, 4, True, {"channels"}, True, False),
}


def _first_iters(sched):
    """Iteration at which the rho of iteration i was first used (plan_rhos' first_iter)."""
    first, out = {}, []
    for i, (rho, _) in enumerate(sched):
        first.setdefault(rho, i)
        out.append(first[rho])
    return out


def _fp_kinds(lib, nw, levels, chan, sched):
    """fp_kind() of every iteration, from admm_plan's rules restated: channel mode; the trajectory kernel where
    effq_admm_uses_traj says so, from traj_after iterations after a change of rho; the bucketed kernel up to 16 levels for
    4096 < nw <= 2^19; else the small kernel up to effq_fp_small_max and the cooperative one above."""
    if chan:
        return ["channels"] * len(sched)
    traj = bool(lib.effq_admm_uses_traj(nw, levels))
    traj_after = 30 if nw > (1 << 20) else 12
    bucket = levels <= 16 and 4096 < nw <= (1 << 19) and nw <= lib.effq_fp_bucket_max()
    older = "bucket" if bucket else ("small" if nw <= lib.effq_fp_small_max() else "coop")
    return ["traj" if traj and i - f >= traj_after else older for i, f in enumerate(_first_iters(sched))]


def _anchor(where, v, wstar, dual_in, alpha, iters, done, G, dual_out, levels, div):
    """The oracle's fixed point and the fp64 restatement of the projection on the loop's own w* and dual of this iteration:
    the bars of tests/test_fp_traj_gpu.py (converged, equal iteration count, alpha within 1e-11) and the equalities of
    tests/test_projection_gpu.py, at the kernel's scale.  Returns the relative deviation of alpha."""
    v, wstar, dual_in = (t.detach().cpu().numpy().reshape(-1) for t in (v, wstar, dual_in))
    assert np.array_equal(_bits(v), _bits(wstar + dual_in)), f"{where}: v is not w* + dual"
    fit = O.fit_scale(torch.from_numpy(v), levels, -1, 1)
    dev_a = abs(alpha - fit.alpha) / fit.alpha
    assert done == 1 and iters == fit.iters and dev_a <= 1e-11, \
        f"{where}: scale {alpha!r} in {iters} iterations (done {done}), oracle {fit.alpha!r} in {fit.iters}"
    _, G_ref, du_ref, _, _ = ref_project(v, wstar, dual_in, alpha, levels, div)
    G, dual_out = G.detach().cpu().numpy().reshape(-1), dual_out.detach().cpu().numpy().reshape(-1)
    assert np.array_equal(_bits(G), _bits(G_ref)), \
        f"{where}: {np.count_nonzero(_bits(G) != _bits(G_ref))} projected weights differ from the fp64 restatement"
    assert np.array_equal(_bits(dual_out), _bits(du_ref)), f"{where}: dual differs from the fp64 restatement"
    return dev_a


PRED_KEYS = ("K", "e", "calls", "warm_iters", "full_iters", "listed", "list_max", "ring_iters", "ring_listed")


@pytest.mark.parametrize("case", list(RUN_CASES))
def test_fused_run_equals_the_step_by_step_ops_on_traj_coop_and_channels(ops, case):
    """effq_admm_run against prox_solve[_shifted] + the fixed point the plan takes + admm_project_dual (channel mode:
    fixed_point_channels with its projection epilogue), 34 iterations: b*, the scale state (scale, iteration count, done;
    channel mode: every row's scale and count) and G of EVERY iteration, then w*, v, the dual and the error flag, in bits.
    Both sides run the same deterministic kernels on the same bits; the one step that differs in code is the K-slice path
    (traj-parts, coop-records-traj: the run adds the slices of the product in the trajectory kernel's prologue, the loop's
    prox_solve in k_prox_reduce4), which test_k_slices_of_the_prox_product_added_up_in_the_prologue shows to sum in the
    same slice order - so nothing is loosened.  The loop carries ONE prediction buffer, as the run does: after the loop the
    two hold the same brackets and the same tallies of warm, wide-bracket and full iterates.  The buffer has no counter of
    trajectory calls (`calls` counts the recorders too): that the trajectory kernel ran at exactly the planned iterations
    is INFERRED from those three tallies, which only it adds to (fp_traj.h) and which must equal the fixed-point iterations
    of the planned trajectory iterations.
    Every case also re-evaluates hist[j] of all 34 slots with conv_step: nine hand-overs to the loss stream on its four
    recycled events (section b's 11 iterations use each event once at most).

    coop-records-traj is the 144 -> 144 layer of the issue (nw = 559 872), not a smaller stand-in."""
    from efficientq_amd.hip_ops import to_ndhwc
    c1, c2, k, levels, chan, classes, split, residuals = RUN_CASES[case]
    lib = ops.lib
    nwrow = c1 * k ** 3
    nw, n = c2 * nwrow, nwrow + 1
    L = _layer(c1, c2, k, seed=c1 + 3 * c2 + k)
    sched = _rho_schedule(L.rho, L.rho_max, ITERS, PERIOD)
    assert [d for _, d in sched] == pytest.approx([2.0] + [1.0] * 15 + [2.0] + [1.0] * 15 + [1.25, 1.0])
    assert [i for i in range(1, ITERS) if sched[i][0] != sched[i - 1][0]] == [1, 17, 33]
    n_inv = lib.effq_admm_num_inverses(L.rho, L.rho_max, ITERS, PERIOD)
    assert n_inv == 3 == len({r for r, _ in sched}) - 1          # both side streams carry an inverse

    # ---- the class this case was built for
    kinds = _fp_kinds(lib, nw, levels, chan, sched)
    assert set(kinds) == classes, (case, sorted(set(kinds)))
    traj_at = [i for i, kd in enumerate(kinds) if kd == "traj"]
    plan = ops.prox_plan(c2, n)
    assert (plan["nsplit"] > 1) == split, plan
    if "traj" in classes:
        assert lib.effq_admm_uses_traj(nw, levels) and traj_at == TRAJ_ITERS and kinds[33] != "traj" and c2 <= 512
        assert nw >= 65536 and (nw > (1 << 19)) == ("coop" in classes) and nw <= (1 << 20)
    else:
        assert chan or not lib.effq_admm_uses_traj(nw, levels)
    if classes == {"coop"}:
        assert nw > lib.effq_fp_small_max() and levels > 16 and nw <= lib.effq_fp_coop_max()
    if chan:
        assert nwrow <= lib.effq_fp_channels_max_row()

    xq, yn = dev(to_ndhwc(L.x)), dev(to_ndhwc(L.y))
    W0, b0 = dev(L.w.reshape(c2, nwrow).contiguous()), dev(L.b)
    A0, B0 = ops.gram(xq, None, yn, L.geom, True)
    run = ops.admm_run(A0, B0, W0, b0, L.geom, yn, xq=xq, rho=L.rho, rho_max=L.rho_max, eta=L.eta, iters=ITERS,
                       period=PERIOD, levels=levels, channel_wise=chan, residuals=residuals)
    torch.cuda.synchronize()
    assert int(run.err.item()) == 0
    assert (run.fp_pred is not None) == ("traj" in classes)

    G = W0.clone()
    dual = torch.zeros_like(W0)
    wstar, v = torch.empty_like(W0), torch.empty_like(W0)
    bstar = torch.empty(c2, device=DEV)
    st, pred = ops.new_fp_state(), ops.new_fp_pred()
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ldb = -(-n // 4) * 4
    Bm = torch.zeros(c2, ldb, device=DEV)                          # (the loop's prox_solve builds its own right-hand side)
    inverses, worst_alpha, worst_res, traj_fp_iters = {}, 0.0, 0.0, 0
    for i, (rho_i, div) in enumerate(sched):
        kind = kinds[i]
        where = f"{case}, iteration {i} (rho {rho_i:g}, dual divisor {div:g}, fixed point: {kind})"
        rho_use = sched[1][0] if i == 0 else rho_i
        if rho_use not in inverses:
            inverses[rho_use] = ops.spd_inverse(A0, True, rho_use, L.eta)
        anchored = kind == "traj" or (i > 0 and sched[i - 1][0] != rho_i)
        dual_in = dual.clone() if anchored else None
        if i == 0:
            ops.prox_solve_shifted(B0, inverses[rho_use], W0, b0, G, dual, rho_i, L.eta, rho_use, wstar, bstar)
        else:
            ops.prox_solve(B0, inverses[rho_use], W0, b0, G, dual, rho_i, L.eta, wstar, bstar)
        Gn = torch.empty_like(W0)
        if chan:
            alpha = torch.zeros(c2, dtype=torch.float64, device=DEV)
            its = torch.zeros(c2, dtype=torch.int32, device=DEV)
            rho_next = sched[i + 1][0] if i + 1 < ITERS else rho_i
            ops.fixed_point_channels(wstar, dual, v, levels, alpha, its, err,
                                     proj=dict(G=Gn, dual_div=div, Bm=Bm, B0=B0, W0=W0, ldb=ldb, rho_next=rho_next,
                                               eta=L.eta))
        else:
            if kind == "traj":
                ops.fixed_point_traj(wstar.view(-1), dual.view(-1), v.view(-1), levels, st, pred)
            elif kind == "bucket":
                ops.fixed_point_bucket_rec(wstar.view(-1), dual.view(-1), v.view(-1), levels, st, pred)
            else:
                ops.fixed_point_coop_rec(wstar.view(-1), dual.view(-1), v.view(-1), levels, st, pred)
            ops.admm_project_dual(v.view(-1), wstar.view(-1), st, levels, Gn.view(-1), dual.view(-1), div)
        torch.cuda.synchronize()
        assert _same(run.b_ring[i], bstar), \
            f"{where}: prox solve, bias column differs by {(run.b_ring[i] - bstar).abs().max().item():.3e}"
        if chan:
            assert _same(run.alpha_ring[i], alpha), \
                f"{where}: row scales differ by {(run.alpha_ring[i] - alpha).abs().max().item():.3e}"
            assert torch.equal(run.w_iters_ring[i], its), f"{where}: fixed-point iteration counts of the rows"
        else:
            a, it, done = ops.read_fp_state(st)
            a_run, it_run, done_run = ops.read_fp_state(run.state_ring[i])
            assert _same(run.state_ring[i, 0:1], st[0:1]) and (it_run, done_run) == (it, done), \
                f"{where}: run's scale {a_run!r} in {it_run} iterations (done {done_run}), loop's {a!r} in {it} ({done})"
            if kind == "traj":
                traj_fp_iters += it
        diff = (run.G_ring[i].view_as(Gn) - Gn).abs().max().item()
        assert _same(run.G_ring[i], Gn), f"{where}: projected weights differ by {diff:.3e}"
        if anchored and chan:
            a_h, it_h = alpha.cpu().tolist(), its.cpu().tolist()
            for r in (0, 1, c2 - 1):
                worst_alpha = max(worst_alpha, _anchor(f"{where}, row {r}", v[r], wstar[r], dual_in[r], a_h[r], it_h[r], 1,
                                                       Gn[r], dual[r], levels, div))
        elif anchored:
            worst_alpha = max(worst_alpha, _anchor(where, v, wstar, dual_in, a, it, done, Gn, dual, levels, div))
        if residuals:
            # k_admm_residuals: non-negative fp64 terms, one rounding per square, summed in whatever order
            w64, g64 = wstar.cpu().numpy().astype(np.float64).reshape(-1), Gn.cpu().numpy().astype(np.float64).reshape(-1)
            p64 = G.cpu().numpy().astype(np.float64).reshape(-1)
            want = (np.sum((w64 - g64) ** 2), np.sum((g64 - p64) ** 2))
            got = run.res[i].cpu().tolist()
            for which, (g_, w_) in enumerate(zip(got, want)):
                if w_ == 0.0:                            # G did not move: every term is an exact zero
                    assert g_ == 0.0, f"{where}: residual {which} {g_!r} where the fp64 sum is 0"
                    continue
                worst_res = max(worst_res, abs(g_ - w_) / ((nw + 2) * U53 * w_))
                assert abs(g_ - w_) <= (nw + 2) * U53 * w_, \
                    f"{where}: residual {which} {g_!r} against {w_!r} ({abs(g_ - w_) / w_:.3e} relative)"
        G = Gn
    assert _same(run.wstar, wstar), "last prox solve, weight columns"
    assert _same(run.v, v), "last projection input"
    assert _same(run.dual, dual), "final dual"
    assert int(err.item()) == 0 and len(inverses) == n_inv
    # ---- hist over the RECYCLED loss events: the forked loss stream (kind 0: the conv pass, groups of 4) is handed the
    # iterates after iterations 3, 7, ... 31 and 33, through event (i / 4) % 4 - nine hand-overs on four events, each event
    # recorded again while the loss stream may still be busy behind its previous record.  hist[j] must still be the
    # stand-alone conv loss of ring slot j, in bits (grid_sum_finish: a fixed order, see section b).
    handovers = [i for i in range(ITERS) if (i + 1) % 4 == 0 or i + 1 == ITERS]
    events = [(i // 4) % 4 for i in handovers]
    assert len(handovers) == 9 and min(events.count(e) for e in range(4)) == 2 and events.count(0) == 3
    hist = run.hist.cpu().numpy()
    for j in range(ITERS):
        _, sq = ops.conv_step(xq, run.G_ring[j], run.b_ring[j], L.geom, yn, None)
        alone = sq.cpu().tolist()[0]
        assert float(hist[j, 0]) == alone and not math.isnan(alone), \
            f"{case}, ring slot {j} (hand-over {j // 4}, event {(j // 4) % 4}): hist {float(hist[j, 0])!r}, conv_step on " \
            f"the slot's own G and b {alone!r}"
    line = f"{TAG} a. {case}: nw = {nw}, n = {n}, prox K slices {plan['nsplit']}, classes " + \
           ", ".join(f"{kd} x {kinds.count(kd)}" for kd in sorted(set(kinds)))
    if "traj" in classes:
        assert nw > 256 * 1024 or not residuals            # the residual kernel's single-pass span is 256 blocks x 1024
        p_run, p_loop = ops.read_fp_pred(run.fp_pred), ops.read_fp_pred(pred)
        assert p_run["calls"] == ITERS and p_run["warm_iters"] > 0, p_run
        # the recorders add nothing to these three tallies: they count the iterates of the trajectory calls alone, each as
        # served by the narrow bracket, by the wide one or by a full pass
        assert p_run["warm_iters"] + p_run["ring_iters"] + p_run["full_iters"] == traj_fp_iters, (p_run, traj_fp_iters)
        for key in PRED_KEYS:
            assert p_run[key] == p_loop[key], (key, p_run, p_loop)
        K = p_run["K"]
        for key in ("lo", "hi", "eps", "eps_n"):
            assert p_run[key][:K] == p_loop[key][:K], (key, p_run, p_loop)
        line += (f"; trajectory calls planned at iterations {traj_at} ({len(traj_at)}); read from the prediction buffer: "
                 f"{p_run['calls']} recorded calls of all kernels, and {p_run['warm_iters']} warm + {p_run['ring_iters']} "
                 f"wide-bracket + {p_run['full_iters']} full iterates, which only the trajectory kernel tallies and which "
                 f"equal the {traj_fp_iters} fixed-point iterations of those {len(traj_at)} iterations: {len(traj_at)} "
                 f"trajectory calls, inferred")
    line += f"; alpha against the oracle: worst {worst_alpha:.2e} relative (bar 1e-11)"
    line += (f"; hist equals conv_step on its own slot in bits over {len(handovers)} hand-overs on 4 events "
             f"({len(set(hist[:, 0].tolist()))} distinct losses of {ITERS})")
    if residuals:
        line += f"; residuals: worst {worst_res:.2e} of the bound (nw + 2) 2^-53"
    print(line)


# ------------------------------------------------------------------ b. hist[j] is the loss of iterate j
L_ITERS, L_PERIOD = 11, 4
# loss kind: (c1, c2, k, activation levels, weight levels, group of the forked loss stream)
LOSS_CASES = {
    0: (4, 8, 3, 4, 4, 4),
    1: (32, 32, 3, 4, 4, 4),          # conv_i8_supported: 3^3 at stride 1, c1 in {32, 64, ...}, c2 a multiple of 32
    2: (4, 32, 3, 4, 256, 4),         # conv_i8s_supported: c1 = 4, one channel tile; 256 weight levels: `prepare` has work
    4: (4, 8, 3, 4, 4, 8),
    5: (64, 32, 1, 4, 4, 8),          # gram_loss_i8_supported: c2 a multiple of 32, nw a multiple of 64
}


def _numerators(Gq, Lw):
    """2 * level - (Lw - 1) from the int8 ring (above 128 levels the ring holds level - 128; csrc/conv3d_i8s.hip)."""
    q = Gq.to(torch.int64)
    return q if Lw <= 128 else 2 * q + (257 - Lw)


@pytest.mark.parametrize("kind", list(LOSS_CASES))
def test_hist_holds_the_loss_of_its_own_iterate(ops, kind):
    """hist[j, 0] of an 11-iteration run (period 4: the forked loss stream takes the iterates in groups of 4 + 4 + 3 for the
    conv kinds and 8 + 3 for the Gram kinds, iteration 0 is the shifted solve; three hand-overs at most, so none of the four
    loss events is used twice here - event reuse is exercised by the 34-iteration runs of section a, which re-evaluate
    their hist the same way) against the stand-alone entry point of the same loss on ring slot j's own G / Gq, b and scale state.

    In bits, for every kind: conv3d_quant_calib_step (0), conv3d_calib_step_i8 (1), conv3d_calib_step_i8s (2) and
    effq_gram_loss (4) assign tiles to workgroups statically and finish with grid_sum_finish (common.h), whose last
    workgroup adds the per-workgroup partials in block order; effq_gram_loss_i8 (5) accumulates its quadratic form with
    INTEGER atomics (exact in any order) and adds the linear terms of every iterate through the same grid_sum_finish, on a
    grid that does not depend on the size of the group.  No kernel ends in fp64 atomics, so the V 2^-53 bar is not needed
    anywhere.  The run with and without the loss stream must give the same bits too.

    Against fp64 on the CPU, sum (conv3d(xq, G_j) + b_j - y)^2, at the bar the kernel's own test holds:
      0: 2e-6 (test_conv_geometry_gpu.py:316)   4: 1e-10 (test_gram_shapes_gpu.py:249)
      1, 2: 3e-6 with the fp32 tensors xq and G_ring[j] as operands (test_conv_geometry_gpu.py:489, the bar between the integer
         kernel and fp32 operands), and 1e-6 with the operands of the integer model the kernels are specified on - xq =
         f32(alpha_a) id / (La - 1), G = f32(alpha_w) (2 level - (Lw - 1)) / (Lw - 1) - as on the line above it (:488)
      5: 2e-8 of |quadratic term| + |rest| (test_gram_shapes_gpu.py:603), with the fp32 tensors as operands and with those of
         the integer model, which is what that line compares with (the fp32 tensors differ from the model by the roundings
         of xq and G to fp32, ~6e-8 of the outputs).
    Kind 2 runs at 256 weight levels: the per-voxel level sums that `prepare` caches exist only above 128; the run prepares
    them at j = 0 only, the re-evaluation at every slot.
    The layers are the smallest 3^3 (kind 5: 1^3) geometry each *_supported query accepts at a whole channel tile, and
    the test asserts that the query refuses the next smaller one.  The seeds are those at which the oracle's
    calibrate_layer (same layer, 11 iterations, period 4) has 11 distinct scales - hence 11 distinct G, whose largest
    magnitude is the scale - and the test requires the 11 ring slots to be pairwise distinct, so a shifted slot index cannot hide in a plateau."""
    from efficientq_amd.hip_ops import to_ndhwc
    c1, c2, k, La, Lw, group = LOSS_CASES[kind]
    nwrow = c1 * k ** 3
    n, V = nwrow + 1, 2 * 6 * 6 * 8
    L = _layer(c1, c2, k, seed=100 + kind)
    geom = L.geom
    from efficientq_amd.hip_ops import make_geom
    smaller = lambda cc1, cc2: make_geom((2, cc1, 6, 6, 8), cc2, k, 1, k // 2)
    if kind == 1:
        assert ops.conv_i8_supported(geom, La, Lw)
        assert not ops.conv_i8_supported(smaller(c1 // 2, c2), La, Lw) and not ops.conv_i8_supported(smaller(c1, c2 // 2), La, Lw)
    if kind == 2:
        assert ops.conv_i8s_supported(geom, La, Lw)
        assert not any(ops.conv_i8s_supported(smaller(cc1, c2), La, Lw) for cc1 in (1, 2, 3))
        # fewer output channels are accepted, as a partly empty channel tile: 32 is the smallest that fills one
        assert ops.conv_i8s_plan(geom, La, Lw)["CT"] == 1 and ops.conv_i8s_plan(smaller(c1, c2 + 1), La, Lw)["CT"] == 2
    if kind == 5:
        assert ops.gram_loss_i8_supported(c2, n, True, Lw) and ops.gram_i8_supported(geom, La)
        assert not ops.gram_loss_i8_supported(c2, n - 32, True, Lw) and not ops.gram_loss_i8_supported(c2 - 16, n, True, Lw)
    sched = _rho_schedule(L.rho, L.rho_max, L_ITERS, L_PERIOD)
    assert [d for _, d in sched] == pytest.approx([2.0, 1, 1, 1, 2.0, 1, 1, 1, 1.25, 1, 1])
    groups = [min(group, L_ITERS - g) for g in range(0, L_ITERS, group)]
    assert groups == ([4, 4, 3] if kind in (0, 1, 2) else [8, 3])

    xn, yn = dev(to_ndhwc(L.x)), dev(to_ndhwc(L.y))
    a_act, _, st_a = ops.fit_scale(xn, La, 0.0, 1.0)
    xq, _, xidx = ops.quant_dequant_f64path(xn, st_a, La, 0.0, 1.0, want_idx=True)
    alpha_act = torch.tensor(a_act, dtype=torch.float32, device=DEV)
    W0, b0 = dev(L.w.reshape(c2, nwrow).contiguous()), dev(L.b)
    kw = {}
    if kind == 4:
        assert ops.gram_f64_supported(geom, True)
        A0, B0 = ops.gram(xq, None, yn, geom, True)
        Au, Bu = ops.gram_f64(xq, yn, geom, True)
        syy = (yn.double() ** 2).sum().reshape(1)
        kw["loss_gram"] = (Au, Bu, syy)
    elif kind == 5:
        A0, B0, Au, Bu = ops.gram_i8(xidx, ops.att_classes(None), yn, geom, True, alpha_act, La, unweighted=True)
        syy = (yn.double() ** 2).sum().reshape(1)
        planes = ops.gram_loss_i8_planes(Au, True, alpha_act, La, V)
        torch.cuda.synchronize()
        assert planes is not None and int(planes._effq_err.item()) == 0
        kw["loss_gram"] = (Au, Bu, syy, planes)
    else:
        A0, B0 = ops.gram(xq, None, yn, geom, True)

    def run_once(overlap):
        r = ops.admm_run(A0, B0, W0, b0, geom, yn, xq=xq, xidx=xidx, act_alpha=alpha_act, act_levels=La,
                         loss_kind=kind if kind in (1, 2) else 0, rho=L.rho, rho_max=L.rho_max, eta=L.eta, iters=L_ITERS,
                         period=L_PERIOD, levels=Lw, overlap=overlap, **kw)
        torch.cuda.synchronize()
        assert int(r.err.item()) == 0
        return r

    run, serial = run_once(True), run_once(False)
    assert _same(run.hist, serial.hist), (run.hist[:, 0].tolist(), serial.hist[:, 0].tolist())
    assert _same(run.G_ring, serial.G_ring) and _same(run.state_ring[:, 0], serial.state_ring[:, 0])
    hist = run.hist.cpu().numpy()
    for j in range(L_ITERS):
        for i in range(j):
            assert not torch.equal(run.G_ring[i], run.G_ring[j]), f"iterates {i} and {j} are the same tensor"

    x64 = xq.cpu().permute(0, 4, 1, 2, 3).double()
    y64 = L.y.double()
    ids64 = xidx.cpu().permute(0, 4, 1, 2, 3).double()
    sa = float(np.float32(a_act)) / (La - 1)
    checks = []
    for j in range(L_ITERS):
        where = f"loss kind {kind}, ring slot {j} (forked groups {groups})"
        Gj, bj, stj = run.G_ring[j], run.b_ring[j], run.state_ring[j]
        a_w = float(stj[0].item())
        if kind == 0:
            _, sq = ops.conv_step(xq, Gj, bj, geom, yn, None)
            alone = sq.cpu().tolist()[0]
        elif kind == 1:
            sq = torch.zeros(2, dtype=torch.float64, device=DEV)
            alone = ops.conv_step_i8(xidx, run.Gq_ring[j], bj, geom, yn, alpha_act, La, stj, Lw, sq).cpu().tolist()[0]
        elif kind == 2:
            sq = torch.zeros(2, dtype=torch.float64, device=DEV)
            alone = ops.conv_step_i8s(xidx, run.Gq_ring[j], bj, geom, yn, alpha_act, La, stj, Lw, sq, True).cpu().tolist()[0]
        elif kind == 4:
            alone = ops.gram_loss(Au, Bu, syy, Gj, bj).cpu().tolist()[0]
        else:
            alone = ops.gram_loss_i8(planes, Au, Bu, syy, run.Gq_ring[j:j + 1].view(1, c2, nwrow), run.b_ring[j:j + 1],
                                     run.state_ring[j:j + 1], alpha_act, La, Lw).cpu().tolist()[0][0]
        assert float(hist[j, 0]) == alone and not math.isnan(alone), \
            f"{where}: hist {float(hist[j, 0])!r}, the stand-alone entry point on the slot's own operands {alone!r}"

        def loss64(xx, GG):
            out = F.conv3d(xx, GG.reshape(c2, c1, k, k, k), None, padding=L.pad)
            full = out + bj.cpu().double().view(1, -1, 1, 1, 1)
            ref = ((full - y64) ** 2).sum().item()
            quad = (out ** 2).sum().item()
            return ref, abs(quad) + abs(ref - quad)

        ref32, mag32 = loss64(x64, Gj.cpu().double())
        got = float(hist[j, 0])
        if kind in (0, 4):
            bar, line = (2e-6, "tests/test_conv_geometry_gpu.py:316") if kind == 0 else (1e-10, "tests/test_gram_shapes_gpu.py:249")
            checks.append((where, "fp32 operands", got, ref32, abs(got - ref32) / (bar * ref32), line))
            continue
        # the int8 ring against the fp32 ring: conv_forward_i8's host formula
        lm1 = Lw - 1
        level = torch.round((Gj / stj[0].to(torch.float32) + 1.0) * (0.5 * lm1)).to(torch.int64)
        m = _numerators(run.Gq_ring[j], Lw)
        assert torch.equal(m, 2 * level - lm1), f"{where}: Gq_ring is not 2 level - (L - 1) of G_ring / alpha"
        G_model = float(np.float32(a_w)) * m.cpu().double() / lm1
        assert (Gj.cpu().double() - G_model).abs().max().item() <= 4 * 2.0 ** -24 * a_w
        ref_m, mag_m = loss64(ids64 * sa, G_model)
        if kind == 5:
            line = "2e-8 (|quadratic| + |rest|), tests/test_gram_shapes_gpu.py:603"
            checks.append((where, "fp32 operands", got, ref32, abs(got - ref32) / (2e-8 * mag32), line))
            checks.append((where, "integer model", got, ref_m, abs(got - ref_m) / (2e-8 * mag_m), line))
        else:
            checks.append((where, "fp32 operands", got, ref32, abs(got - ref32) / (3e-6 * ref32),
                           "3e-6, tests/test_conv_geometry_gpu.py:489"))
            checks.append((where, "integer model", got, ref_m, abs(got - ref_m) / (1e-6 * ref_m),
                           "1e-6, tests/test_conv_geometry_gpu.py:488"))
    worst = {what: max(c[4] for c in checks if c[1] == what) for what in sorted({c[1] for c in checks})}
    print(f"{TAG} b. loss kind {kind}: {c1} -> {c2}, {k}^3, {La} / {Lw} levels, groups {groups}: hist equals the "
          f"stand-alone entry point in bits on 11 distinct iterates; worst deviation from fp64 as a fraction of the bar: " +
          ", ".join(f"{what} {w:.3e}" for what, w in worst.items()))
    for where, what, got, ref, frac, line in checks:
        assert frac <= 1.0, f"{where}: hist {got!r}, fp64 on the {what} {ref!r}: {frac:.3e} of the bar ({line})"


# ------------------------------------------------------------------ c. best-iterate selection
NAN = float("nan")
HISTORIES = {
    "strictly-decreasing": [9.0, 8.0, 7.5, 7.25, 7.0, 6.5],
    "minimum-twice": [9.0, 3.0, 5.0, 3.0, 4.0, 8.0],
    "minimum-first": [1.0, 3.0, 1.0, 2.0, 1.5, 1.0],
    "nan-later": [5.0, 4.0, NAN, 3.0, NAN, 6.0],
    "nan-first": [NAN, 4.0, 2.0, 3.0, 1.0, 6.0],
    "decoys-in-column-1": [6.0, 5.0, 2.0, 7.0, 2.5, 3.0],
}
WANT_INDEX = {"strictly-decreasing": 5, "minimum-twice": 1, "minimum-first": 0, "nan-later": 3, "nan-first": 0,
              "decoys-in-column-1": 2}


def _reference_best(losses):
    """EfficientQConv.py:139-142, literally."""
    best = best_i = None
    for i, loss in enumerate(losses):
        if i == 0 or loss < best:
            best, best_i = loss, i
    return best, best_i


@pytest.mark.parametrize("has_b", [True, False], ids=["bias", "no-bias"])
@pytest.mark.parametrize("c2", [1, 257])
@pytest.mark.parametrize("nw", [5, 4096, 262144 + 3])
def test_best_iterate_selection_equals_the_reference_loop(ops, nw, c2, has_b):
    """effq_admm_select_best on a hand-built run handle: ring element e of slot s holds s + e / 2^19 (exact in fp32 and
    different for every (s, e)), so a copy from the wrong slot, a mixed copy or a missed tail shows.  262 147 weights are one
    pass of the 1024 x 256 grid plus three elements of the stride loop; c2 = 257 is a bias row of two blocks' worth."""
    iters = 6
    e = torch.arange(nw, dtype=torch.float64) / 2.0 ** 19
    G_ring = (torch.arange(iters, dtype=torch.float64)[:, None] + e[None, :]).float()
    assert torch.equal(G_ring.double(), torch.arange(iters, dtype=torch.float64)[:, None] + e[None, :])
    b_ring = (100.0 + torch.arange(iters, dtype=torch.float64)[:, None] + torch.arange(c2)[None, :] / 512.0).float()
    alpha_ring = (torch.arange(iters, dtype=torch.float64)[:, None] * 3.0 + torch.arange(c2)[None, :] / 1024.0)
    run = SimpleNamespace(iters=iters, nw=nw, c2=c2, has_b=has_b, G_ring=dev(G_ring), b_ring=dev(b_ring) if has_b else None,
                          alpha_ring=dev(alpha_ring))
    for name, losses in HISTORIES.items():
        want_loss, want_i = _reference_best(losses)
        assert want_i == WANT_INDEX[name]
        hist = torch.zeros(iters, 2, dtype=torch.float64)
        hist[:, 0] = torch.tensor(losses, dtype=torch.float64)
        if name == "decoys-in-column-1":                    # every odd double is smaller than every loss, smallest first
            hist[:, 1] = torch.tensor([-6.0, -5.0, -4.0, -3.0, -2.0, -1.0], dtype=torch.float64)
        run.hist = dev(hist)
        best_G, best_b, best = ops.admm_select_best(run)
        torch.cuda.synchronize()
        got_loss, got_i = best.cpu().tolist()
        assert got_i == float(want_i), (name, got_i, want_i)
        assert (math.isnan(got_loss) and math.isnan(want_loss)) or got_loss == want_loss, (name, got_loss, want_loss)
        assert _same(best_G, run.G_ring[want_i]), (name, "best_G is not ring slot", want_i)
        if has_b:
            assert _same(best_b, run.b_ring[want_i]), (name, "best_b is not ring slot", want_i)
        else:
            assert best_b is None
        assert _same(ops.channel_alpha_best(run, best), run.alpha_ring[want_i]), name


# ------------------------------------------------------------------ d. the packed Gram system
@pytest.mark.parametrize("c2", [1, 64])
@pytest.mark.parametrize("n", [2, 65, 1500])
def test_gram_pack_and_unpack_carry_the_upper_triangle_only(ops, n, c2):
    """gram_reduce with an identity and with a doubling reducer: the message is A0's upper triangle in np.triu order, then
    B0, in bits; unpacking mirrors it, whatever the lower triangle held (here: something else).  n = 1500 takes the
    grid-stride loop (n^2 + c2 n > 8192 x 256)."""
    assert (n * n + c2 * n > 8192 * 256) == (n == 1500)
    rng = np.random.default_rng(n + c2)
    A = rng.standard_normal((n, n)).astype(np.float32)
    A[np.tril_indices(n, -1)] = -7.5                             # deliberately not the mirror of the upper triangle
    B = rng.standard_normal((c2, n)).astype(np.float32)
    iu = np.triu_indices(n)
    assert ops.lib.effq_gram_packed_elems(n, c2) == iu[0].size + c2 * n
    for factor in (1.0, 2.0):
        A0, B0 = dev(torch.from_numpy(A.copy())), dev(torch.from_numpy(B.copy()))
        seen = []

        def reducer(buf):
            seen.append(buf.clone())
            if factor != 1.0:
                buf.mul_(factor)

        ops.gram_reduce(A0, B0, reducer)
        torch.cuda.synchronize()
        assert len(seen) == 1
        assert np.array_equal(_bits(seen[0].cpu().numpy()), _bits(np.concatenate([A[iu], B.reshape(-1)])))
        mirror = np.triu(A) + np.triu(A, 1).T
        assert np.array_equal(_bits(A0.cpu().numpy()), _bits((factor * mirror).astype(np.float32)))
        assert torch.equal(A0, A0.T)
        assert np.array_equal(_bits(B0.cpu().numpy()), _bits((factor * B).astype(np.float32)))
