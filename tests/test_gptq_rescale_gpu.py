"""--gptq_rescale on the device: effq_gptq_rescale against gptq.rescale_host fed with the sweep's own ids, its guards, and the
layer."""
import numpy as np
import pytest
import torch

from tests.gptq_refine_ref import ETA, system
from tests.test_gptq_refine_gpu import _device_inputs, _layer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# 8 times the worst relative deviation of alpha, b and err from rescale_host over these cases on the MI355X (DESIGN section
# 33.2: 5.9e-13, in err at 16 levels, where f is a small difference of its terms; alpha stays within 3e-15): both sides are
# fp64 on the same fp32-valued inputs and differ in the order of their sums
TOL = 8 * 5.9e-13
# (c2, n, bias): one row in one block; the bias alone in the last block; rows that fill neither a 16-row tile nor a 32-row
# group, with a second group; four column blocks, i.e. tiles on both sides of a diagonal one
SHAPES = [(1, 64, False), (5, 65, True), (33, 130, True), (16, 193, False)]


def _swept(c2, n, bias, levels, per_row, u=None):
    """(ops, the device's inputs and sweep state, the host's inputs) of a system of gptq_refine_ref, u replaced on request."""
    from efficientq_amd import ops_gptq as OG
    from efficientq_amd.qconv import get_ops
    A0, H, u0, alpha = system(n, bias, c2, per_row)
    u = u0 if u is None else u
    ops, (A, u_w, u_b, a) = get_ops(DEV), _device_inputs(A0, u, alpha, bias)
    P = OG.gptq_chol(ops, A, ETA, read_flag=True)
    G, b, ids, _, row_flag = OG.gptq_sweep(ops, P, n, u_w, u_b, a, levels, want_ids=True, per_row=per_row)
    return ops, (A, u_w, u_b, a, G, b, ids, row_flag, OG.gptq_flag(P, n)), (H, u, alpha)


def _rescale(ops, dev, levels, per_row, pd_flag=None):
    from efficientq_amd import ops_gptq as OG
    A, u_w, u_b, a, G, b, ids, row_flag, flag = dev
    a, G, b = a.clone(), G.clone(), None if b is None else b.clone()
    err, kept = OG.gptq_rescale(ops, A, ETA, u_w, u_b, a, levels, G, b, ids, row_flag, flag if pd_flag is None else pd_flag,
                                per_row=per_row, out=(torch.full((G.shape[0],), 7.0, dtype=torch.float64, device=DEV),
                                                      torch.zeros(1, dtype=torch.int32, device=DEV)))
    return a.cpu(), G.cpu(), None if b is None else b.cpu(), err.cpu(), int(kept.item())


@pytest.mark.parametrize("per_row", [True, False], ids=["rows", "tensor"])
@pytest.mark.parametrize("levels", [4, 16])
@pytest.mark.parametrize("c2,n,bias", SHAPES)
def test_kernel_matches_the_host_rule(c2, n, bias, levels, per_row):
    from efficientq_amd import gptq, ops_gptq as OG
    ops, dev, (H, u, alpha) = _swept(c2, n, bias, levels, per_row)
    plan, nb = OG.gptq_rescale_plan(ops, c2, n), -(-n // 64)
    assert (plan["nblk"], plan["tiles"], plan["runs"], plan["launches"]) == (nb, nb * (nb + 1) // 2, nb * (nb + 1) // 2, 3)
    assert plan["forms_grid"] == plan["runs"] * -(-c2 // 32)
    ids, b0 = dev[6].cpu(), (dev[5].double().cpu().numpy() if bias else None)
    want_a, want_b, want_err, want_kept = gptq.rescale_host(H, u, ids.numpy(), b0, alpha, levels, bias, per_row)
    a, G, b, err, kept = _rescale(ops, dev, levels, per_row)
    dev_a = np.abs(a.numpy() - want_a) / want_a
    dev_e = np.abs(err.numpy() - want_err) / want_err
    dev_b = np.abs(b.double().numpy() - want_b) / np.abs(want_b) if bias else np.zeros(1)
    print(f"c2={c2} n={n} bias={bias} L={levels} rows={per_row}: alpha {dev_a.max():.3e} err {dev_e.max():.3e} b {dev_b.max():.3e}")
    assert kept == want_kept == 0 and not np.array_equal(a.numpy(), np.broadcast_to(alpha, a.shape))
    assert dev_a.max() <= TOL and dev_e.max() <= TOL and dev_b.max() <= TOL + 2.0 ** -24   # b leaves the device in fp32
    d = 2.0 / (levels - 1)
    a32 = a.float().reshape(-1, 1)
    assert torch.equal(G, a32 * ((ids.double() * d - 1.0).float() if per_row else ids.float() * d - 1))
    again = _rescale(ops, dev, levels, per_row)                      # equal bits from equal inputs
    assert all(x is y or torch.equal(x, y) for x, y in zip((a, G, b, err), again[:4]))


def test_guards_keep_the_row_bit_for_bit():
    """A zero row of u with equal ids and a pre-flagged row keep alpha, G and b and are counted; a set pd_flag leaves
    every output untouched."""
    _, _, u, _ = system(130, True, 5, True)
    u = u.copy()
    u[1] = 0.0
    ops, dev, _ = _swept(5, 130, True, 4, True, u=u)
    dev[6][1] = 2                                                     # one level: v H v^T > 0 and v H u^T = 0
    dev = dev[:7] + (torch.tensor([0, 0, 0, 1, 0], dtype=torch.int32, device=DEV),) + dev[8:]
    a, G, b, err, kept = _rescale(ops, dev, 4, True)
    a0, G0, b0 = dev[3].cpu(), dev[4].cpu(), dev[5].cpu()
    bad, good = [1, 3], [0, 2, 4]
    assert kept == 2 and err[3] == 7.0 and bool((err[good + [1]] != 7.0).all())
    assert torch.equal(a[bad], a0[bad]) and torch.equal(G[bad], G0[bad]) and torch.equal(b[bad], b0[bad])
    assert bool((a[good] != a0[good]).all()) and bool((b[good] != b0[good]).all())
    a, G, b, err, kept = _rescale(ops, dev, 4, True, pd_flag=torch.ones(1, dtype=torch.int32, device=DEV))
    assert kept == 0 and bool((err == 7.0).all()) and torch.equal(a, a0) and torch.equal(G, G0) and torch.equal(b, b0)


@pytest.mark.parametrize("channel_wise", [False, True], ids=["tensor", "rows"])
def test_layer(channel_wise):
    """32 -> 32 at 3^3 on 16^3 voxels, 4 / 4 levels: the refit does not raise the sweep's error nor its pass the refit's (to
    the 1e-9 that the fp32 rounding of the committed G and b may cost); the weights survive the round trip through the
    stored ids; without rounds the layer is the one built without the argument."""
    plain, zero = _layer(lwq_channel_wise=channel_wise), _layer(lwq_channel_wise=channel_wise, gptq_rescale=0)
    conv = _layer(lwq_channel_wise=channel_wise, gptq_rescale=1, gptq_refine=1)
    assert torch.equal(plain.weight.data, zero.weight.data) and torch.equal(plain.bias.data, zero.bias.data)
    t0, t = zero.last_trace, conv.last_trace
    assert (t0["gptq_rescale"], t0["gptq_kept"]) == (0, 0) and t0["gptq_err_rescaled"] == t0["gptq_err"] == plain.last_trace["gptq_err"]
    print(f"sweep {t['gptq_err_sweep']!r} refit {t['gptq_err_rescaled']!r} pass {t['gptq_err']!r}")
    assert (t["gptq_rescale"], t["gptq_kept"]) == (1, 0) and t["gptq_err_sweep"] == t0["gptq_err"]
    assert 0.0 < t["gptq_err"] <= t["gptq_err_rescaled"] * (1 + 1e-9) and t["gptq_err_rescaled"] <= t["gptq_err_sweep"] * (1 + 1e-9)
    assert np.any(np.asarray(t["alpha_w"]) != np.asarray(t0["alpha_w"]))
    w = conv.weight.data.clone()
    conv.store_int_weight()
    conv.weight.data = conv.weight.data.to(DEV)
    conv.restore_fp_weight()
    assert torch.equal(conv.weight.data, w)
