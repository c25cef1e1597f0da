"""TEST-ONLY restatement of the calibrator's channel mode (lwq_channel_wise: one weight scale per output channel) on the
CPU, built from the oracle's primitives without changing them:

- ``fit_rows``: ``oracle.fit_scale`` on every output row, with the rule for a row whose values are all zero (scale 0,
  0 iterations, levels (L-1)//2, weights 0: the reference formula would divide by zero there);
- ``calibrate_layer_channels``: ``oracle.calibrate_layer``'s loop order (prox solve through ``oracle.ProxSystem``,
  projection, dual update, conv + MSE, rho schedule, earliest-best selection) with the per-row projection; it keeps the
  BEST iterate's scales.  ``dtype=torch.float64`` is the anchor mode, as in the oracle;
- ``ChannelOracleOps``: ``tests/cpu_backend.OracleOps`` (subclassed, not edited) with channel mode in ``admm_run``, so
  the product's host code (qconv.EfficientQConvHIP.ptq) runs on the CPU.
"""
from types import SimpleNamespace
from typing import List, Optional

import torch
import torch.nn.functional as F

from oracle import effq_oracle as O
from tests.cpu_backend import OracleOps


def fit_rows(v: torch.Tensor, levels: int):
    """Per-row project_by_iter of v ([c2, ...]): (alphas [c2] python doubles, iters [c2], b64 [c2, nwrow] fp64 levels)."""
    rows = v.detach().double().reshape(v.shape[0], -1)
    alphas, iters, bs = [], [], []
    for r in rows:
        if float(r.abs().sum()) == 0.0:
            alphas.append(0.0)
            iters.append(0)
            bs.append(torch.full_like(r, O.level_step(levels, -1.0, 1.0) * ((levels - 1) // 2) - 1.0))
            continue
        f = O.fit_scale(r, levels, -1.0, 1.0)
        alphas.append(f.alpha)
        iters.append(f.iters)
        bs.append(f.b64)
    return alphas, iters, torch.stack(bs)


def project_rows(v: torch.Tensor, levels: int, dtype=torch.float32):
    """G = alpha_c * b per row, in the calibrator's arithmetic: fp32(alpha_c) * fp32(b) (fp64 in anchor mode); 0 on a zero
    row.  Returns (G shaped like v, alphas, iters)."""
    alphas, iters, b64 = fit_rows(v, levels)
    a = torch.tensor(alphas, dtype=torch.float64).unsqueeze(1)
    if dtype == torch.float64:
        G = a * b64
    else:
        G = a.float() * b64.float()
    G = torch.where(a == 0, torch.zeros_like(G), G)
    return G.reshape(v.shape).to(dtype), alphas, iters


def calibrate_layer_channels(x, y_fp, weight, bias, stride, padding, qlvl_w=4, qlvl_act=4, q_act=True,
                             mask_pyramid=None, iters=O.ADMM_ITERS, dtype=torch.float32):
    """oracle.calibrate_layer with one weight scale per output channel (see the module docstring)."""
    f64 = dtype == torch.float64
    x = x.detach().to(dtype)
    y_fp = y_fp.detach().to(dtype)
    G = weight.detach().to(dtype)
    if bias is not None:
        bias = bias.detach().to(dtype)
    if mask_pyramid is not None and f64:
        mask_pyramid = [m.to(dtype) for m in mask_pyramid]
    dual = torch.zeros_like(G)
    rho_scale = max(y_fp.numel() * y_fp.std().item() / (G.numel() * G.std().item()), 1.0)
    att = O.pick_mask(mask_pyramid, y_fp.shape)
    if att is not None:
        rho_scale *= att.mean().item()
    alpha_act = None
    if q_act:
        fit = O.fit_scale(x, qlvl_act, 0.0, 1.0)
        alpha_act = fit.alpha
        xq = fit.alpha * (fit.b64 if f64 else fit.b)
    else:
        xq = x
    rho, rho_cap, eta = O.RHO0 * rho_scale, O.RHO_MAX * rho_scale, O.ETA0 * rho_scale
    k = tuple(int(i) for i in weight.shape[2:])
    sysm = O.ProxSystem(xq, y_fp, k, stride, padding, G.clone(), bias.clone() if bias is not None else None, att,
                        dtype=dtype)
    best = None
    losses, alphas_hist, iters_hist = [], [], []
    wstar0 = None
    bstar = bias
    for i in range(iters):
        wstar, bs = sysm.solve(rho, eta, G - dual)
        if bias is not None:
            bstar = bs
        if i == 0:
            wstar0 = wstar.clone()
        G, a_c, it_c = project_rows(wstar + dual, qlvl_w, dtype)
        dual = wstar - G + dual
        out_q = F.conv3d(xq, G, bstar, stride, padding)
        loss = F.mse_loss(out_q, y_fp).item()
        losses.append(loss)
        alphas_hist.append(a_c)
        iters_hist.append(it_c)
        if i % O.RHO_PERIOD == 0:
            if rho * 2 <= rho_cap:
                rho *= 2
                dual = dual / 2
            else:
                dual = dual / (rho_cap / rho)
                rho = rho_cap
        if i == 0 or loss < best[2]:
            best = (G, bstar if bias is not None else None, loss, i)
    Gb, Bb, _, bi = best
    out_q = F.conv3d(xq, Gb, Bb, stride, padding)
    final = F.mse_loss(out_q, y_fp).item()
    if att is not None:
        final = (att.unsqueeze(1) * ((out_q - y_fp) ** 2)).mean().item()
    return SimpleNamespace(weight=Gb, bias=Bb, alpha_w=alphas_hist[bi], alpha_act=alpha_act, layer_loss=final,
                           best_iter=bi, loss_history=losses, alpha_w_history=alphas_hist, w_iters_history=iters_hist,
                           wstar0=wstar0, qact=xq)


class ChannelOracleOps(OracleOps):
    """OracleOps with the channel mode of effq_admm_run (per-row fixed points; alpha ring; best iterate's scales)."""

    def admm_run(self, A0, B0, W0, b0, geom, y_ndhwc, *, xq=None, xidx=None, act_alpha=None, act_levels=0,
                 loss_kind=0, rho, rho_max, eta, iters, period, levels, overlap=True, residuals=False,
                 channel_wise=False):
        if not channel_wise:
            return super().admm_run(A0, B0, W0, b0, geom, y_ndhwc, xq=xq, xidx=xidx, act_alpha=act_alpha,
                                    act_levels=act_levels, loss_kind=loss_kind, rho=rho, rho_max=rho_max, eta=eta,
                                    iters=iters, period=period, levels=levels, overlap=overlap, residuals=residuals)
        assert loss_kind in (0, 4)
        has_b = b0 is not None
        c2 = B0.shape[0]
        G = W0.clone()
        dual = torch.zeros_like(W0)
        wstar = torch.empty_like(W0)
        r = SimpleNamespace(iters=iters, nw=W0.numel(), c2=c2, has_b=has_b, G_ring=[], b_ring=[] if has_b else None,
                            hist=torch.zeros(iters, 2, dtype=torch.float64), channel_wise=True, alpha_ring=[],
                            w_iters_ring=[], res=None)
        for i in range(iters):
            A = self.spd_inverse(A0, has_b, rho, eta)
            bstar = torch.empty(c2) if has_b else None
            self.prox_solve(B0, A, W0, b0, G, dual, rho, eta, wstar, bstar)
            Gn, a_c, it_c = project_rows(wstar + dual, levels)
            d = wstar - Gn + dual
            if i % period == 0:
                dual_div = 2.0 if rho * 2 <= rho_max else rho_max / rho
                d = d / dual_div
            dual = d
            _, sq = self.conv_step(xq, Gn, bstar, geom, y_ndhwc)
            r.hist[i] = sq
            r.G_ring.append(Gn)
            r.alpha_ring.append(a_c)
            r.w_iters_ring.append(it_c)
            if has_b:
                r.b_ring.append(bstar)
            G = Gn
            if i % period == 0:
                rho = rho * 2 if rho * 2 <= rho_max else rho_max
        return r

    @staticmethod
    def admm_read(run, best, extra=None):
        if not getattr(run, "channel_wise", False):
            return OracleOps.admm_read(run, best, extra)
        bi = int(best[1])
        w_iters = [max(it) for it in run.w_iters_ring]
        w_rows = [max(range(run.c2), key=lambda c: it[c]) for it in run.w_iters_ring]
        return dict(hist=run.hist[:, 0].tolist(), best=best.tolist(), alpha_w=list(run.alpha_ring[bi]), w_iters=w_iters,
                    w_iters_rows=w_rows, err=0, extra=extra.double().reshape(-1).tolist() if extra is not None else None)

    # storage helpers the product calls (bit packing as in the library: little-endian bit stream)
    @staticmethod
    def storage_bits(levels):
        return 1 if levels <= 2 else 2 if levels <= 4 else 4 if levels <= 16 else 8

    def pack_levels(self, idx, bits):
        v = idx.to(torch.int64).reshape(-1)
        per = 8 // bits
        pad = (-v.numel()) % per
        v = torch.cat([v, torch.zeros(pad, dtype=torch.int64)]).reshape(-1, per)
        sh = torch.arange(per, dtype=torch.int64) * bits
        return (v << sh).sum(dim=1).to(torch.uint8)

    def unpack_levels(self, packed, n, bits):
        per = 8 // bits
        sh = torch.arange(per, dtype=torch.int64) * bits
        v = (packed.to(torch.int64).unsqueeze(1) >> sh) & ((1 << bits) - 1)
        return v.reshape(-1)[:n].to(torch.uint8)


def install(monkeypatch):
    import efficientq_amd.qconv as Q
    ops = ChannelOracleOps()
    monkeypatch.setattr(Q, "get_ops", lambda device: ops)
    return ops


def rows_on_grid(w: torch.Tensor, alpha: torch.Tensor, levels: int, tol: float = 1e-6) -> bool:
    """Every row c of w lies on alpha_c * {2j/(L-1) - 1} (relative to alpha_c; zero rows: all zero)."""
    a = alpha.reshape(-1).double()
    w = w.reshape(w.shape[0], -1).double()
    ok = True
    for c in range(w.shape[0]):
        if a[c] == 0:
            ok &= bool((w[c] == 0).all())
            continue
        u = (w[c] / a[c] + 1) * (levels - 1) / 2
        ok &= bool(((u - u.round()).abs() <= tol * (levels - 1)).all()) and bool((u.round() >= 0).all()) and \
            bool((u.round() <= levels - 1).all())
    return ok
