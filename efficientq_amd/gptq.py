"""One-pass layer calibration by sequential rounding with error feedback (OBQ / GPTQ, Babai's nearest plane):
``--qconv gptq``, the cheap companion of the 200-iteration ADMM calibrator of qconv.py.

The rule, per layer with n = k^3 c1 (+ 1) unknowns per output row, weights in the reference's layout, the bias last:

1. H = A0 + eta I, eta = lwq_eta * rho_scale: the Hessian of  ||Y - [W|b] X||^2_att + eta ||[W|b] - [W0|b0]||^2.
   Its minimiser is u* = (B0 + eta [W0|b0]) H^-1 (effq_spd_inverse and effq_prox_solve at rho = 0).
2. The weight scale is project_by_iter on the weight part of u* (per tensor, or per row with lwq_channel_wise) and stays fixed.
3. H = P P^T with P upper triangular: the Cholesky factor of the index-reversed matrix, fp64.
4. Per output row, with s = 0, for j = 0 .. n-1:
       t_j = u*_j - s_j / P_jj
       q_j = alpha * disc64(t_j, alpha, -1, 1, 2 / (L - 1))   for a weight,   q_j = t_j   for the bias
       s_k += (q_j - u*_j) P_jk  for k > j,     err += (P_jj (q_j - t_j))^2
   t_j minimises the quadratic form over column j with the earlier columns at their rounded values and the later ones
   free; err ends as (q - u*) H (q - u*)^T.  Only P is needed, not the factor of H^-1.
5. The rounded weights, the bias and the scale go through the calibrator's own final forward and commit.

``factor_host`` / ``sweep_host`` state 3 and 4 in numpy the way the kernels of csrc/gptq.hip walk them - reversed indices,
64-column blocks, the later columns' s updated once per block - for the tests and for reading; ``GPTQConvHIP`` is the layer.

Two optional steps around 4 (``--gptq_refine K``, ``--gptq_order act``; both off by default):

4a. Activation ordering: the weight columns are visited by descending diag(A0) (``order_host``), the bias still last: A0
    and u* are permuted, factor, sweep and passes run on the permuted system, G and the ids are scattered back.  The scale
    of 2 is fitted before and does not depend on the order.
4b. K passes of coordinate descent on the same quadratic form (``refine_host``, csrc/gptq_refine.hip), from the sweep's
    result q, with g = (q - u*) H.  A pass visits j = 0 .. n-1:
        t = q_j - g_j / H_jj
        q' = alpha * disc64(t)  for a weight,   q' = t  for the bias
        a weight moves only if (q' - t)^2 < (q_j - t)^2, the bias always;  on a move  g += (q' - q_j) H[j, :],  q_j = q'
    A move lowers the row's error by H_jj ((q_j - t)^2 - (q' - t)^2), so no pass raises it; err = sum_j g_j (q_j - u*_j).

And one around 2 (``--gptq_rescale R``, off by default): the scale of 2 is an unweighted fit and never sees H.
4c. R rounds of [refit, then the K passes of 4b on the new grid]: with the level ids fixed, v_j = id_j d - 1, a row is
    q = [alpha v | beta] and its error  f(alpha, beta) = alpha^2 a11 + 2 alpha beta a12 + beta^2 a22 - 2 alpha c1 - 2 beta c2 + c0
    with a11 = v H_ww v^T, a12 = v . H_wb, a22 = H_bb, c1 = v . (H u*^T)_w, c2 = (H u*^T)_b, c0 = u* H u*^T.  The refit
    (``rescale_host``, csrc/gptq_rescale.hip) is the minimiser of f: per row the 2 x 2 solve, per tensor one alpha for the
    summed f and every row's own beta.  It is taken only where it is a finite positive scale from a positive denominator,
    so neither a refit nor a pass raises the error: a block-coordinate descent on the layer's own objective.
"""
from __future__ import annotations

import time
from types import SimpleNamespace

import numpy as np
import torch

from . import ops_gptq
from .qconv import (GRAM_LOSS_DEFAULT, GRAM_LOSS_I8_MAX_N, GRAM_LOSS_MAX_N, EfficientQConvHIP, _call_if, layer_paths)


def disc64(t, alpha, levels: int):
    """(value, level id) of t on the grid alpha * (2 i / (L - 1) - 1): layer_helper.py:25-37 in fp64."""
    d = 2.0 / (levels - 1)
    idx = np.rint((np.clip(t / alpha, -1.0, 1.0) + 1.0) / d)
    return idx * d - 1.0, idx


def factor_host(H: np.ndarray) -> np.ndarray:
    """P upper triangular with H = P P^T."""
    return np.linalg.cholesky(H[::-1, ::-1])[::-1, ::-1]


def sweep_host(P: np.ndarray, u: np.ndarray, alpha, levels: int, has_bias: bool, block: int = ops_gptq.BLOCK):
    """(q, ids, err) of the rule for u (c2, n) and alpha (a scalar or c2 scales), walked as the device walks it."""
    c2, n = u.shape
    npad = -(-n // block) * block
    L = np.eye(npad)
    L[:n, :n] = P[::-1, ::-1]
    ur = np.zeros((c2, npad))
    ur[:, :n] = u[:, ::-1]
    a = np.broadcast_to(np.asarray(alpha, dtype=np.float64).reshape(-1), (c2,))
    S, q, ids, err = np.zeros((c2, npad)), np.zeros((c2, npad)), np.zeros((c2, npad)), np.zeros(c2)
    for B in range(npad // block - 1, -1, -1):
        kb = B * block
        delta = np.zeros((c2, block))
        for jj in range(min(block, n - kb) - 1, -1, -1):
            j = kb + jj
            t = ur[:, j] - S[:, j] / L[j, j]
            if has_bias and j == 0:
                qj = t
            else:
                v, ids[:, j] = disc64(t, a, levels)
                qj = a * v
            err += (L[j, j] * (qj - t)) ** 2
            delta[:, jj] = qj - ur[:, j]
            S[:, kb:j] += np.outer(delta[:, jj], L[j, kb:j])
            q[:, j] = qj
        S[:, :kb] += delta @ L[kb:kb + block, :kb]
    return q[:, :n][:, ::-1], ids[:, :n][:, ::-1], err


def refine_host(H: np.ndarray, u: np.ndarray, ids, b, alpha, levels: int, has_bias: bool, passes: int,
                block: int = ops_gptq.BLOCK):
    """(q, ids, moves, err, margin) after `passes` passes of rule 4b over the sweep's state - the level ids (c2, n - has_bias)
    and the bias b (c2) - walked as the device walks it: 64-column blocks in natural order, g step by step inside a
    block, the columns outside it once per block.  err: (passes, c2), the error after every pass.  margin: per row the
    smallest margin of a decision, as a difference of squared distances in units of alpha^2: of an acceptance whose grid
    value differs from the current one, |(q' - t)^2 - (q_j - t)^2|, and of the rounding of an unclipped t, 2 d times its
    distance from the boundary between two levels."""
    c2, n = u.shape
    nw = n - int(has_bias)
    a = np.broadcast_to(np.asarray(alpha, dtype=np.float64).reshape(-1), (c2,))
    d = 2.0 / (levels - 1)
    ids = np.array(ids, dtype=np.float64).reshape(c2, nw)
    q = np.empty((c2, n))
    q[:, :nw] = a[:, None] * (ids * d - 1.0)
    if has_bias:
        q[:, -1] = np.asarray(b, dtype=np.float64)
    g = (q - u) @ H
    moves, margin, errs = np.zeros(c2, dtype=np.int64), np.full(c2, np.inf), []
    for _ in range(passes):
        for kb in range(0, n, block):
            ke = min(kb + block, n)
            delta = np.zeros((c2, ke - kb))
            for j in range(kb, ke):
                t = q[:, j] - g[:, j] / H[j, j]
                if has_bias and j == n - 1:
                    dl, q[:, j] = t - q[:, j], t
                else:
                    v, idx = disc64(t, a, levels)
                    qn = a * v
                    gain = (q[:, j] - t) ** 2 - (qn - t) ** 2
                    take = gain > 0.0
                    x = (t / a + 1.0) / d
                    edge = np.where((x > 0.0) & (x < levels - 1), 2.0 * d * d * np.abs(np.abs(x - np.floor(x)) - 0.5), np.inf)
                    margin = np.minimum(margin, np.minimum(edge, np.where(idx != ids[:, j], np.abs(gain) / a ** 2, np.inf)))
                    dl = np.where(take, qn - q[:, j], 0.0)
                    q[:, j] = np.where(take, qn, q[:, j])
                    ids[:, j] = np.where(take, idx, ids[:, j])
                    moves += take
                delta[:, j - kb] = dl
                g[:, kb:ke] += np.outer(dl, H[j, kb:ke])
            g[:, :kb] += delta @ H[kb:ke, :kb]
            g[:, ke:] += delta @ H[kb:ke, ke:]
        errs.append(np.einsum("rj,rj->r", g, q - u))
    return q, ids, moves, np.array(errs), margin


def rescale_host(H: np.ndarray, u: np.ndarray, ids, b, alpha, levels: int, has_bias: bool, per_row: bool, row_flag=None):
    """(alpha, b, err, kept) of rule 4c for the level ids (c2, n - has_bias), the bias b (c2, or None) and the scale(s)
    alpha the rows stand on.  With the bias eliminated, num_r = c1 - a12 c2 / a22 and den_r = a11 - a12^2 / a22 (c1 and a11
    without a bias): alpha_r = num_r / den_r per row, alpha = sum_r num_r / sum_r den_r per tensor (the rows added in row
    order), beta_r = (c2 - a12 alpha) / a22.  A refit is taken only if its denominator is positive, alpha finite and
    positive, beta finite and the row not flagged (row_flag, or a present scale that is not finite and positive); per
    tensor every row must pass.  Where it is not taken the row keeps alpha and b, and kept counts it (rows, or 1 for the
    tensor).  err: f at the point every row stands on afterwards (without meaning for a flagged row)."""
    c2, n = u.shape
    nw = n - int(has_bias)
    v = np.zeros((c2, n))
    v[:, :nw] = np.asarray(ids, dtype=np.float64).reshape(c2, nw) * (2.0 / (levels - 1)) - 1.0
    a_old = np.broadcast_to(np.asarray(alpha, dtype=np.float64).reshape(-1), (c2,))
    b_old = np.asarray(b, dtype=np.float64).reshape(c2) if has_bias else np.zeros(c2)
    vH, uH = v @ H, u @ H
    a11, c1, c0 = (np.einsum("rj,rj->r", x, y) for x, y in ((vH, v), (vH, u), (uH, u)))
    if has_bias:
        a12, cb, a22 = vH[:, -1], uH[:, -1], H[-1, -1]
        num, den = c1 - a12 * cb / a22, a11 - a12 * a12 / a22
    else:
        a12, cb, a22, num, den = np.zeros(c2), np.zeros(c2), 0.0, c1, a11
    live = np.isfinite(a_old) & (a_old > 0.0)
    if row_flag is not None:
        live &= np.asarray(row_flag).reshape(c2) == 0
    with np.errstate(all="ignore"):
        if per_row:
            a_new = num / den
        else:
            N = D = 0.0
            for r in range(c2):
                N, D = N + num[r], D + den[r]
            a_new, den = np.full(c2, N / D), np.full(c2, D)
        beta_new = (cb - a12 * a_new) / a22 if has_bias else np.zeros(c2)
        take = live & (den > 0.0) & np.isfinite(a_new) & (a_new > 0.0) & np.isfinite(beta_new)
    if not per_row:
        take = np.full(c2, bool(take.all()))
    a, beta = np.where(take, a_new, a_old), np.where(take, beta_new, b_old)
    err = a * a * a11 + 2.0 * a * beta * a12 + beta * beta * a22 - 2.0 * a * c1 - 2.0 * beta * cb + c0
    kept = int((~take).sum()) if per_row else int(not take[0])
    return (a if per_row else a[:1]), (beta if has_bias else None), err, kept


def order_host(diag_a0, has_bias: bool) -> np.ndarray:
    """The visiting order of ``--gptq_order act``: the weight columns by descending diag(A0), ties in their own order,
    the bias last."""
    diag_a0 = np.asarray(diag_a0)
    nw = diag_a0.shape[0] - int(has_bias)
    perm = np.argsort(-diag_a0[:nw], kind="stable")
    return np.concatenate([perm, [nw]]) if has_bias else perm


def round_columns(ops, A0, eta, u_w, u_b, alpha, levels, per_row, refine=0, order="natural", rescale=0):
    """Steps 3, 4 and 4a to 4c on the device, nothing read back: (G, b, ids, err, err_sweep, moves, row_flag, pd_flag, P,
    err_rescaled, kept).  err_sweep is the sweep's error and err the final one (the same tensor without passes or
    refits); moves is None without passes; ids is None unless passes or refits ran.  rescale = R: R rounds of [refit,
    `refine` passes]; alpha is then updated in place, err_rescaled is the error after the last refit and kept counts the
    refits not taken (both None without)."""
    n = int(A0.shape[0])
    perm = None
    if order == "act":
        perm = ops_gptq.gptq_order(A0, u_b is not None)
        up = torch.triu(A0)                                   # the triangle the kernels read, mirrored: a full matrix to permute
        A0 = (up + torch.triu(A0, 1).T)[perm][:, perm].contiguous()
        u_w = u_w[:, perm[:u_w.shape[1]]].contiguous()
    P = ops_gptq.gptq_chol(ops, A0, eta)
    pd_flag = ops_gptq.gptq_flag(P, n)
    err_rescaled = kept = None
    if rescale:
        G, b, ids, err_sweep, row_flag = ops_gptq.gptq_sweep(ops, P, n, u_w, u_b, alpha, levels, want_ids=True, per_row=per_row)
        err, moves, kept = err_sweep, None, torch.zeros(1, dtype=torch.int32, device=G.device)
        for _ in range(rescale):
            err_rescaled, _ = ops_gptq.gptq_rescale(ops, A0, eta, u_w, u_b, alpha, levels, G, b, ids, row_flag, pd_flag,
                                                    per_row=per_row, out=(torch.empty_like(err_sweep), kept))
            err = err_rescaled
            if refine:
                err, m = ops_gptq.gptq_refine(ops, A0, eta, u_w, u_b, alpha, levels, refine, G, b, ids, row_flag, pd_flag,
                                              per_row=per_row)
                moves = m if moves is None else moves + m
    elif refine:
        G, b, ids, err_sweep, row_flag = ops_gptq.gptq_sweep(ops, P, n, u_w, u_b, alpha, levels, want_ids=True, per_row=per_row)
        err, moves = ops_gptq.gptq_refine(ops, A0, eta, u_w, u_b, alpha, levels, refine, G, b, ids, row_flag, pd_flag,
                                          per_row=per_row)
    else:
        G, b, ids, err, row_flag = ops_gptq.gptq_sweep(ops, P, n, u_w, u_b, alpha, levels, per_row=per_row)
        err_sweep, moves = err, None
    if perm is not None:
        back = torch.empty_like(perm[:G.shape[1]])
        back[perm[:G.shape[1]]] = torch.arange(G.shape[1], device=perm.device)
        G = G[:, back].contiguous()
        ids = ids[:, back].contiguous() if ids is not None else None
    return G, b, ids, err, err_sweep, moves, row_flag, pd_flag, P, err_rescaled, kept


GPTQ_ORDERS = ("natural", "act")


class GPTQConvHIP(EfficientQConvHIP):
    """The layer of ``--qconv gptq``: the statistics, input quantisation, Gram system, final forward and commit of
    EfficientQConvHIP around the rule above instead of the ADMM run.  One host synchronisation per layer.  ``alpha_w`` is the
    one fitted scale (per tensor or per row): the committed weights lie exactly on its grid.  ``gptq_refine=K`` (0 .. 16)
    adds K coordinate-descent passes behind the sweep, ``gptq_order='act'`` visits the columns by descending diag(A0),
    ``gptq_rescale=R`` (0 .. 8) runs R rounds of [scale refit on the quadratic form, the K passes]; ``alpha_w`` is then the
    last refitted scale."""

    def __init__(self, *args, **kwQ):
        super().__init__(*args, **kwQ)
        self.gptq_refine, self.gptq_order, self.gptq_rescale = check_options(
            kwQ.get('gptq_refine', 0), kwQ.get('gptq_order', 'natural'), kwQ.get('gptq_rescale', 0))

    def ptq(self, x):
        c = self._layer_inputs(x)
        ops, red = c.ops, c.red
        rho_scale, y_dim, att, sx, syy_local = self._statistics(c)
        # (no per-iteration losses: the unweighted Gram system behind them is not formed)
        paths = layer_paths(ops, c.geom, self.qlvl_act, self.qlvl_w, c.has_b, c.c2, c.n_sys, c.voxels, q_act=self.q_act,
                            act_inited=self._act_inited, exact_int=self.lwq_exact_int, channel_wise=self.channel_wise,
                            gram_loss_enabled=GRAM_LOSS_DEFAULT, gram_loss_max_n=GRAM_LOSS_MAX_N,
                            gram_loss_i8_max_n=GRAM_LOSS_I8_MAX_N)._replace(losses=None)
        att_cls = ops.att_classes(att) if paths.gram_i8 else None
        paths = paths.after(att_classes_ok=att_cls is not None)
        xq, xidx, act_iters = self._quantise_input(c, sx, paths.want_idx)
        eta = self.lwq_eta * rho_scale
        A0, B0, _, paths = self._gram_system(c, paths, xq, xidx, att, att_cls, syy_local)
        t0 = time.perf_counter()
        fit = self._gptq_run(c, A0, B0, eta)
        fin = self._final_forward(c, paths, fit.run, fit.best, fit.G, fit.b, xq, xidx, att)
        red(fin)
        info = self._gptq_read(fit, fin)                                    # ONE host sync for the layer
        t_fit = time.perf_counter() - t0
        _call_if(ops, "release_retired")
        self._commit(c, fit.G, fit.b, info["alpha_w"])
        numel = y_dim * 1.0
        lossf = (info["fin"][1] if att is not None else info["fin"][0]) / numel
        if self.lwq_verbose:
            passes = (f'err after the sweep = {info["gptq_err_sweep"]:.6g}, after {self.gptq_refine} passes '
                      f'({info["gptq_moves"]} moves) = {info["gptq_err"]:.6g}' if self.gptq_refine else
                      f'err = {info["gptq_err"]:.6g}')
            if self.gptq_rescale:
                passes = (f'err after the sweep = {info["gptq_err_sweep"]:.6g}, after the last of {self.gptq_rescale} scale '
                          f'refits ({info["gptq_kept"]} not taken) = {info["gptq_err_rescaled"]:.6g}, after its '
                          f'{self.gptq_refine} passes ({info["gptq_moves"]} moves in all) = {info["gptq_err"]:.6g}')
            print(f'GPTQ {self.name}: n = {c.n_sys}, eta = {eta:.4f}, scale fit {info["w_iters"]} iterations, '
                  f'{passes}, loss = {lossf:.7f}.')
        if self.layer_loss is not None:
            self.layer_loss.append(f'{self.name:45s}:{lossf}')
        self.last_trace = dict(method='gptq', rho_scale=rho_scale, gptq_err=info["gptq_err"],
                               final_mse=info["fin"][0] / numel, layer_loss=lossf, act_iters=act_iters,
                               w_iters=info["w_iters"], alpha_w=info["alpha_w"], loss_history=[],
                               exact_gram=paths.gram_i8, gptq_s=t_fit, channel_wise=self.channel_wise,
                               paths=paths._asdict(), gptq_refine=self.gptq_refine, gptq_order=self.gptq_order,
                               gptq_err_sweep=info["gptq_err_sweep"], gptq_moves=info["gptq_moves"],
                               gptq_rescale=self.gptq_rescale, gptq_err_rescaled=info["gptq_err_rescaled"],
                               gptq_kept=info["gptq_kept"])

    def _gptq_run(self, c, A0, B0, eta):
        """Steps 1 - 4, enqueued on the current stream; nothing is read back."""
        ops, dev, c2, L = c.ops, c.dev, c.c2, self.qlvl_w
        nw = c.n_sys - int(c.has_b)
        Ainv = ops.spd_inverse(A0, c.has_b, 0.0, eta)
        zero = torch.zeros(c2 * nw, dtype=torch.float32, device=dev)      # G - dual of the prox right-hand side
        u_w = torch.empty(c2, nw, dtype=torch.float32, device=dev)
        u_b = torch.empty(c2, dtype=torch.float32, device=dev) if c.has_b else None
        ops.prox_solve(B0, Ainv, c.W0, c.b0, zero, zero, 0.0, eta, u_w, u_b)
        fp_err = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.channel_wise:
            alpha = torch.empty(c2, dtype=torch.float64, device=dev)
            iters = torch.zeros(c2, dtype=torch.int32, device=dev)
            ops.fixed_point_channels(u_w, None, None, L, alpha, iters, fp_err)
            state = None
        else:
            state = ops.new_fp_state()
            ops.fixed_point_bucket(u_w, None, None, L, state)
            ops.fp_check(state, fp_err)
            alpha, iters = state[:1], state[4:5].view(torch.int32)[:1]
        # (a refit writes the new scale into alpha, i.e. into the state the final forward reads)
        G, b, _, err, err_sweep, moves, row_flag, pd_flag, P, err_rescaled, kept = round_columns(
            ops, A0, eta, u_w, u_b, alpha, L, self.channel_wise, self.gptq_refine, self.gptq_order, self.gptq_rescale)
        # what _final_forward reads of an ADMM run: the scale state of the chosen iterate (the i8 forward folds it in)
        run = SimpleNamespace(state_ring=state.reshape(1, 5)) if state is not None else None
        best = torch.zeros(2, dtype=torch.float64, device=dev)
        return SimpleNamespace(G=G.reshape(-1), b=b, err=err, err_sweep=err_sweep, moves=moves, alpha=alpha, iters=iters,
                               fp_err=fp_err, row_flag=row_flag, pd_flag=pd_flag, run=run, best=best,
                               err_rescaled=err_rescaled, kept=kept, keep=(P, u_w, u_b, Ainv, zero))

    def _gptq_read(self, fit, fin):
        """The layer's one device->host copy; raises naming the layer on what the device flagged."""
        c2 = fit.err.numel()
        f64 = torch.float64
        pack = torch.cat([fin.to(f64).reshape(-1), fit.err, fit.alpha.reshape(-1), fit.iters.to(f64), fit.fp_err.to(f64),
                          fit.pd_flag.to(f64), fit.row_flag.to(f64)] +
                         ([fit.err_sweep, fit.moves.to(f64) if fit.moves is not None else torch.zeros_like(fit.err)]
                          if fit.moves is not None or fit.kept is not None else []) +
                         ([fit.err_rescaled, fit.kept.to(f64)] if fit.kept is not None else [])).cpu().tolist()
        na, ni = fit.alpha.numel(), fit.iters.numel()
        o = 2 + c2
        alpha, iters = pack[o:o + na], pack[o + na:o + na + ni]
        fp_err, pd_flag = (int(v) for v in pack[o + na + ni:o + na + ni + 2])
        rows = [r for r, v in enumerate(pack[o + na + ni + 2:o + na + ni + 2 + c2]) if v]
        # with passes or refits: the sweep's errors, the moves; with refits: the errors after the last one, the count not taken
        tail = pack[o + na + ni + 2 + c2:]
        if pd_flag:
            raise RuntimeError(f'{self.name}: the Gram system A0 + eta I is not positive definite (a pivot of its fp64 '
                               f'Cholesky factorisation was <= 0 or not finite)')
        if fp_err == 2:                                                     # layer_helper.py:62-64
            raise RuntimeWarning(f'{self.name}: Exceed maximum iteration ({100 * self.qlvl_w}) for alpha optimization')
        if fp_err:
            raise RuntimeError(f'{self.name}: weight-scale fixed point did not finish (device state {fp_err})')
        if rows:
            raise RuntimeError(f'{self.name}: the weight scale of output channel(s) {rows[:8]} is not finite and positive')
        err = float(sum(pack[2:o]))
        return dict(fin=pack[:2], gptq_err=err, alpha_w=alpha if self.channel_wise else alpha[0], w_iters=[int(max(iters))],
                    gptq_err_sweep=float(sum(tail[:c2])) if tail else err, gptq_moves=int(sum(tail[c2:2 * c2])),
                    gptq_err_rescaled=float(sum(tail[2 * c2:3 * c2])) if fit.kept is not None else err,
                    gptq_kept=int(tail[3 * c2]) if fit.kept is not None else 0)


def _count(value, top: int) -> bool:
    try:
        return not isinstance(value, bool) and int(value) == value and 0 <= int(value) <= top
    except (TypeError, ValueError):
        return False


def check_options(refine, order, rescale=0):
    """(passes, order, rounds) of ``gptq_refine`` / ``gptq_order`` / ``gptq_rescale``; passes outside 0 .. 16, an unknown
    order, rounds outside 0 .. 8 or more than one round without passes are refused by name."""
    if not _count(refine, ops_gptq.REFINE_MAX_PASSES):
        raise ValueError(f'gptq_refine {refine!r}: the passes behind the sweep, 0 to {ops_gptq.REFINE_MAX_PASSES}')
    if order not in GPTQ_ORDERS:
        raise ValueError(f'gptq_order {order!r}: one of {", ".join(GPTQ_ORDERS)}')
    if not _count(rescale, ops_gptq.RESCALE_MAX_ROUNDS):
        raise ValueError(f'gptq_rescale {rescale!r}: the rounds of [scale refit, passes], 0 to {ops_gptq.RESCALE_MAX_ROUNDS}')
    if int(rescale) > 1 and int(refine) == 0:
        raise ValueError(f'gptq_rescale {rescale!r} with gptq_refine 0: a second refit of unchanged ids changes nothing, '
                         f'give 1 round or passes between the refits')
    return int(refine), order, int(rescale)
