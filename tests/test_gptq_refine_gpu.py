"""--gptq_refine / --gptq_order on the device: effq_gptq_refine against gptq.refine_host fed with the same sweep output,
the activation ordering against the host pipeline on the permuted system, and the layer."""
import numpy as np
import pytest
import torch

from tests.gptq_ref import gptq_ref
from tests.gptq_refine_ref import CASES, ETA, EXCUSED, quad, system, threshold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _device_inputs(A0, u, alpha, bias):
    uf = torch.from_numpy(u.astype(np.float32))
    return (torch.from_numpy(A0).to(DEV), uf[:, :u.shape[1] - int(bias)].contiguous().to(DEV),
            uf[:, -1].contiguous().to(DEV) if bias else None, torch.from_numpy(alpha).to(DEV))


def _sweep_then_refine(A0, u, alpha, levels, bias, passes, per_row=False):
    """The device's sweep state as numpy (ids, b, err) and what gptq_refine made of it (G, b, ids, err, moves)."""
    from efficientq_amd import ops_gptq as OG
    from efficientq_amd.qconv import get_ops
    ops, (A, u_w, u_b, a) = get_ops(DEV), _device_inputs(A0, u, alpha, bias)
    P = OG.gptq_chol(ops, A, ETA, read_flag=True)
    G, b, ids, err, row_flag = OG.gptq_sweep(ops, P, A.shape[0], u_w, u_b, a, levels, want_ids=True, per_row=per_row)
    state = (ids.cpu().numpy(), b.double().cpu().numpy() if bias else None, err.cpu().numpy())
    e, moves = OG.gptq_refine(ops, A, ETA, u_w, u_b, a, levels, passes, G, b, ids, row_flag, OG.gptq_flag(P, A.shape[0]),
                              per_row=per_row)
    return state, (G.cpu(), b.double().cpu().numpy() if bias else None, ids.cpu(), e.cpu().numpy(), moves.cpu().numpy())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n=%d,bias=%d,c2=%d,L=%d,rows=%d,K=%d" % c)
def test_passes_match_the_host_walk(case):
    """ids, moves and b equal refine_host on every row whose decisions all keep the margin of gptq_refine_ref.threshold; err
    is the quadratic form of what came back, to the 1e-9 the sweep's error is held to, and not above the sweep's; after 16
    passes one more host pass accepts no move."""
    from efficientq_amd import gptq, ops_gptq as OG
    from efficientq_amd.qconv import get_ops
    n, bias, c2, levels, per_row, passes = case
    A0, H, u, alpha = system(n, bias, c2, per_row)
    plan, nb = OG.gptq_refine_plan(get_ops(DEV), c2, n, passes), -(-n // 64)
    assert (plan["nblk"], plan["update_gx"]) == (nb, nb) and plan["block_grid"] == {1: 1, 5: 2, 70: 18}[c2]
    assert plan["update_gy"] == {1: 1, 5: 1, 70: 2}[c2] and plan["launches"] == 2 + nb + passes * (2 * nb if nb > 1 else 1)
    (ids0, b0, err0), (G, b, ids, err, moves) = _sweep_then_refine(A0, u, alpha, levels, bias, passes, per_row)
    q_h, ids_h, moves_h, _, margin = gptq.refine_host(H, u, ids0, b0, alpha, levels, bias, passes)
    keep = margin >= threshold(H, q_h, u, alpha, passes)
    print(f"{case}: host moves {int(moves_h.sum())}, err {err0.sum():.6g} -> {err.sum():.6g}, rows left out {int((~keep).sum())}")
    assert moves_h.sum() >= 1 and (~keep).sum() <= EXCUSED * c2 and int(ids.max()) <= levels - 1
    d = 2.0 / (levels - 1)
    a32 = torch.from_numpy(np.broadcast_to(alpha, (c2,)).astype(np.float32)).reshape(c2, 1)
    assert torch.equal(G, a32 * ((ids.double() * d - 1.0).float() if per_row else ids.float() * d - 1))
    q = np.broadcast_to(alpha, (c2,))[:, None] * (ids.numpy().astype(np.float64) * d - 1.0)
    want = quad(H, np.concatenate([q, b[:, None]], axis=1) if bias else q, u)
    assert np.all(np.abs(err - want) <= 1e-9 * want) and np.all(err <= err0 * (1 + 1e-9))
    assert np.array_equal(ids.numpy()[keep], ids_h[keep]) and np.array_equal(moves[keep], moves_h[keep])
    if bias:       # b leaves the device in fp32: half an ulp on top of the 1e-9 of the fp64 value
        assert np.all(np.abs(b - q_h[:, -1])[keep] <= (1e-9 + 2.0 ** -24) * np.abs(q_h[keep, -1]))
    if passes == 16:
        q, _, more, _, margin = gptq.refine_host(H, u, ids.numpy(), b, alpha, levels, bias, 1)
        assert moves.sum() >= 1 and np.all(more[margin >= threshold(H, q, u, alpha, 16)] == 0)


def test_a_flagged_row_and_a_flagged_factor_leave_every_output_untouched():
    from efficientq_amd import ops_gptq as OG
    from efficientq_amd.qconv import get_ops
    A0, _, u, _ = system(130, True, 5, True)
    ops = get_ops(DEV)
    A, u_w, u_b, a = _device_inputs(A0, u, np.array([0.4, 0.0, 0.3, float("nan"), 0.35]), True)
    P = OG.gptq_chol(ops, A, ETA, read_flag=True)
    zeros = torch.zeros(5, dtype=torch.int32, device=DEV)
    for pd_flag, bad in ((OG.gptq_flag(P, 130), [1, 3]), (torch.ones(1, dtype=torch.int32, device=DEV), [0, 1, 2, 3, 4])):
        G, b, ids, err, moves = (torch.full(s, 7, dtype=t, device=DEV) for s, t in (
            ((5, 129), torch.float32), ((5,), torch.float32), ((5, 129), torch.uint8), ((5,), torch.float64), ((5,), torch.int32)))
        row_flag = OG.gptq_sweep(ops, P, 130, u_w, u_b, a, 4, out=(G, b, ids, err, zeros.clone()))[4]
        assert row_flag.cpu().tolist() == [0, 1, 0, 1, 0]
        if len(bad) == 5:          # a flagged factor: the state a sweep on it would have left untouched
            G, b, ids, err = G.fill_(7), b.fill_(7), ids.fill_(7), err.fill_(7)
        OG.gptq_refine(ops, A, ETA, u_w, u_b, a, 4, 2, G, b, ids, row_flag, pd_flag, out=(err, moves))
        good = [r for r in range(5) if r not in bad]
        for t in (G, b, ids, err, moves):
            assert bool((t[bad] == 7).all()) and not (good and bool((t[good] == 7).all()))


def test_activation_order_equals_the_host_pipeline_on_the_permuted_system():
    from efficientq_amd import gptq
    from efficientq_amd.qconv import get_ops
    n, c2, levels, passes = 193, 5, 4, 2
    A0, H, u, alpha = system(n, True, c2, False)
    perm = gptq.order_host(A0.diagonal(), True)
    Hp, up = H[perm][:, perm], u[:, perm]
    _, q, ids_h, _, m_sweep = gptq_ref(Hp, up, alpha, levels, True)
    q, ids_h, _, _, margin = gptq.refine_host(Hp, up, ids_h[:, :-1], q[:, -1], alpha, levels, True, passes)
    keep = (m_sweep >= 1e-8) & (margin >= threshold(Hp, q, up, alpha, passes))
    assert (~keep).sum() <= EXCUSED * c2
    A, u_w, u_b, a = _device_inputs(A0, u, alpha, True)
    G, b, ids, *_ = gptq.round_columns(get_ops(DEV), A, ETA, u_w, u_b, a, levels, False, refine=passes, order="act")
    back = np.empty(n - 1, dtype=np.int64)
    back[perm[:-1]] = np.arange(n - 1)
    assert np.array_equal(ids.cpu().numpy()[keep], ids_h[:, back][keep])
    assert torch.equal(G.cpu(), torch.tensor(np.float32(alpha[0])) * (ids.cpu().float() * (2.0 / (levels - 1)) - 1))
    assert np.all(np.abs(b.double().cpu().numpy() - q[:, -1])[keep] <= (1e-9 + 2.0 ** -24) * np.abs(q[keep, -1]))


def _layer(**kw):
    from efficientq_amd import gptq
    gen = torch.Generator().manual_seed(5)
    c, S = 32, 16
    conv = gptq.GPTQConvHIP(c, c, 3, 1, 1, 1, 1, True, q_weight=True, qlvl=4, q_act=True, qlvl_act=4, **kw)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (2.0 / (c * 27)) ** 0.5)
        conv.bias.copy_(torch.randn(c, generator=gen) * 0.1)
    x_fp = torch.relu(torch.randn(1, c, S, S, S, generator=gen))
    y = torch.nn.functional.conv3d(x_fp, conv.weight.data, conv.bias.data, 1, 1)
    x = torch.relu(x_fp + 0.05 * torch.randn(x_fp.shape, generator=gen))
    conv.output_fp, conv.name, conv.layer_loss = y.to(DEV), "l", []
    conv.to(DEV)
    conv.set_quantizing()
    with torch.no_grad():
        conv(x.to(DEV))
    return conv


@pytest.mark.parametrize("channel_wise", [False, True], ids=["tensor", "rows"])
def test_layer(channel_wise):
    """32 -> 32 at 3^3 on 16^3 voxels, 4 / 4 levels: two passes do not raise the sweep's error, which is that of the layer
    without passes; the weights survive the round trip through the stored ids; the defaults trace no moves."""
    plain, conv = _layer(lwq_channel_wise=channel_wise), _layer(lwq_channel_wise=channel_wise, gptq_refine=2)
    t0, t2 = plain.last_trace, conv.last_trace
    assert (t0["gptq_refine"], t0["gptq_order"], t0["gptq_moves"]) == (0, "natural", 0) and t0["gptq_err_sweep"] == t0["gptq_err"]
    assert (t2["gptq_refine"], t2["gptq_order"]) == (2, "natural") and t2["gptq_moves"] >= 1
    assert t2["gptq_err_sweep"] == t0["gptq_err"] and 0.0 < t2["gptq_err"] <= t2["gptq_err_sweep"]
    w = conv.weight.data.clone()
    conv.store_int_weight()
    assert conv.weight.data.dtype == torch.uint8 and int(conv.weight.data.max()) <= 3
    conv.weight.data = conv.weight.data.to(DEV)
    conv.restore_fp_weight()
    assert torch.equal(conv.weight.data, w)
