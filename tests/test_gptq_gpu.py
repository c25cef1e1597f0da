"""--qconv gptq on the device: effq_gptq_chol and effq_gptq_sweep against the plain fp64 rule of tests/gptq_ref.py, the layer
and the mission.  Inputs are exact in fp32 (integer X, dyadic u*), so both sides see the same numbers."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.gptq_ref import gptq_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ETA = 8.0
# (c2, c1, k, bias, levels, per-row scales): below one block; n = 65, one column past a block edge, with and without the
# bias as that column; rows that do not fill a tile; n = 433; n = 1729 (28 blocks); per-row scales
CASES = [(1, 1, 3, True, 4, False), (4, 1, 3, False, 4, False), (4, 64, 1, True, 2, False), (4, 65, 1, False, 4, False),
         (33, 2, 3, True, 16, False), (8, 16, 3, True, 4, False), (33, 16, 3, True, 256, False),
         (5, 64, 3, True, 4, False), (6, 3, 3, True, 8, True)]


@functools.lru_cache(maxsize=None)
def _system(n, bias, seed=0):
    """(A0 fp32, H fp64): A0 = 2 X^T X of integers in -3 .. 3 over 4 n rows (a ones column for the bias), exact in fp32."""
    rng = np.random.default_rng(1000 * seed + n)
    X = rng.integers(-3, 4, (4 * n, n)).astype(np.float64)
    if bias:
        X[:, -1] = 1.0
    A0 = 2.0 * X.T @ X
    assert np.abs(A0).max() < 2 ** 24
    return A0.astype(np.float32), A0 + ETA * np.eye(n)


@functools.lru_cache(maxsize=None)
def _case(c2, c1, k, bias, levels, per_row):
    n = k ** 3 * c1 + int(bias)
    A0, H = _system(n, bias)
    rng = np.random.default_rng(7 * n + c2)
    u = rng.integers(-511, 512, (c2, n)) / 1024.0
    alpha = 0.3 + 0.02 * np.arange(c2) if per_row else np.array([0.4])
    return n, A0, H, u, alpha, gptq_ref(H, u, alpha, levels, bias)


def _ops():
    from efficientq_amd.qconv import get_ops
    return get_ops(DEV)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "c2=%d,c1=%d,k=%d,bias=%d,L=%d,rows=%d" % c)
def test_sweep_matches_the_fp64_rule(case):
    """Both sides are fp64 and differ by summation order only (about n cond 2^-53, below 1e-11 of a level), so the level ids
    are equal wherever the reference keeps 1e-8 from a rounding boundary; at most one row per case may fail that."""
    from efficientq_amd import ops_gptq as OG
    c2, c1, k, bias, levels, per_row = case
    n, A0, H, u, alpha, (P_ref, q, ids, err, margin) = _case(*case)
    ops = _ops()
    plan = OG.gptq_plan(ops, c2, n)
    assert plan["nblk"] == -(-n // 64) and plan["block_grid"] == -(-c2 // 4) and plan["trail_gy"] == -(-c2 // 64)
    assert plan["sweep_launches"] == 2 * plan["nblk"] and plan["chol_launches"] == 3 * plan["nblk"] - 1
    P = OG.gptq_chol(ops, torch.from_numpy(A0).to(DEV), ETA, read_flag=True)
    nw = n - int(bias)
    uf = torch.from_numpy(u.astype(np.float32))
    assert np.array_equal(uf.double().numpy(), u)
    u_b = uf[:, -1].contiguous().to(DEV) if bias else None
    G, b, got_ids, got_err, row_flag = OG.gptq_sweep(ops, P, n, uf[:, :nw].contiguous().to(DEV), u_b,
                                                     torch.from_numpy(alpha).to(DEV), levels, want_ids=True)
    keep = margin >= 1e-8
    print(f"{case}: smallest margin {margin.min():.3g}, rows left out {int((~keep).sum())}")
    assert (~keep).sum() <= 1 and int(row_flag.abs().sum()) == 0
    assert np.array_equal(got_ids.cpu().numpy()[keep], ids[:, :nw][keep])
    e = got_err.cpu().numpy()
    assert np.all(np.abs(e - err)[keep] <= 1e-9 * err[keep]), np.abs(e / err - 1).max()
    if bias:       # b leaves the device in fp32: half an ulp on top of the 1e-9 of the fp64 value
        qb = q[:, -1]
        assert np.all(np.abs(b.cpu().numpy().astype(np.float64) - qb)[keep] <= (1e-9 + 2.0 ** -24) * np.abs(qb[keep]))
    # the committed weight: f32(alpha) times the level value, in the arithmetic that restores a stored weight
    d = 2.0 / (levels - 1)
    a32 = torch.from_numpy(np.broadcast_to(alpha, (c2,)).astype(np.float32)).reshape(c2, 1)
    lv = got_ids.cpu()
    val = (lv.double() * d - 1.0).float() if per_row else lv.float() * d - 1
    assert torch.equal(G.cpu(), a32 * val)


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[5], CASES[7]], ids=["n=28", "n=65", "n=433", "n=1729"])
def test_chol_factor(case):
    from efficientq_amd import ops_gptq as OG
    n, A0, H, _, _, ref = _case(*case)
    ops = _ops()
    assert OG.gptq_plan(ops, 1, n)["nblk"] == {28: 1, 65: 2, 433: 7, 1729: 28}[n]
    Pf = OG.gptq_chol(ops, torch.from_numpy(A0).to(DEV), ETA, read_flag=True)
    assert int(OG.gptq_flag(Pf, n).cpu()) == 0
    P = OG.gptq_factor(Pf, n).cpu().numpy()
    assert np.array_equal(P, np.triu(P)) and P.diagonal().min() > 0.0
    resid = np.abs(P @ P.T - H).max()
    print(f"n = {n}: max|P P^T - H| = {resid:.3g} (bound {n * 2.0 ** -50 * np.abs(H).max():.3g}), "
          f"max|P - ref| = {np.abs(P - ref[0]).max():.3g}")
    assert resid <= n * 2.0 ** -50 * np.abs(H).max()


def test_indefinite_matrix_is_flagged_and_the_sweep_writes_nothing():
    from efficientq_amd import _lib, ops_gptq as OG
    n, A0, _, u, alpha, _ = _case(*CASES[2])
    A0 = A0.copy()
    A0[40, 40] = -100.0
    ops = _ops()
    with pytest.raises(_lib.EffqError, match="EFFQ_ERR_NOT_SPD"):
        OG.gptq_chol(ops, torch.from_numpy(A0).to(DEV), ETA, read_flag=True)
    P = OG.gptq_chol(ops, torch.from_numpy(A0).to(DEV), ETA)
    assert int(OG.gptq_flag(P, n).cpu()) == 1
    c2, nw = u.shape[0], n - 1
    out = (torch.full((c2, nw), 7.0, device=DEV), torch.full((c2,), 7.0, device=DEV),
           torch.full((c2, nw), 7, dtype=torch.uint8, device=DEV), torch.full((c2,), 7.0, dtype=torch.float64, device=DEV),
           torch.full((c2,), 7, dtype=torch.int32, device=DEV))
    uf = torch.from_numpy(u.astype(np.float32))
    OG.gptq_sweep(ops, P, n, uf[:, :nw].contiguous().to(DEV), uf[:, -1].contiguous().to(DEV),
                  torch.from_numpy(alpha).to(DEV), 2, out=out)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)


def test_bad_arguments_are_refused_and_a_bad_scale_flags_its_row():
    from efficientq_amd import _lib, ops_gptq as OG
    n, A0, _, u, _, _ = _case(*CASES[1])
    ops = _ops()
    A = torch.from_numpy(A0).to(DEV)
    for eta in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(_lib.EffqError, match="EFFQ_ERR_ARG"):
            OG.gptq_chol(ops, A, eta)
    P = OG.gptq_chol(ops, A, ETA)
    uw = torch.from_numpy(u.astype(np.float32)).to(DEV)
    for levels in (1, 257):
        with pytest.raises(_lib.EffqError):
            OG.gptq_sweep(ops, P, n, uw, None, torch.tensor([0.4], dtype=torch.float64, device=DEV), levels)
    alpha = torch.tensor([0.4, 0.0, float("nan"), 0.4], dtype=torch.float64, device=DEV)
    G = torch.full((4, n), 7.0, device=DEV)
    out = OG.gptq_sweep(ops, P, n, uw, None, alpha, 4, out=(G, None, None, torch.zeros(4, dtype=torch.float64, device=DEV),
                                                          torch.zeros(4, dtype=torch.int32, device=DEV)))
    assert out[4].cpu().tolist() == [0, 1, 1, 0]
    assert bool((G[1:3] == 7).all()) and bool((G[0] != 7).all()) and bool((G[3] != 7).all())


@pytest.mark.parametrize("levels", [4, 16])
@pytest.mark.parametrize("channel_wise", [False, True], ids=["tensor", "rows"])
def test_layer(levels, channel_wise):
    """A GPTQConvHIP 8 -> 8 at 3^3 on 2 x 12^3: the committed weights are alpha_w times grid values and survive the round
    trip through the stored level ids bit for bit; layer_loss is the loss of an fp64 conv of the committed weights on the
    quantised input to the fp32 rounding of the conv epilogue (2e-6, the bound of
    test_layer_gpu.test_losses_from_the_gram_system_equal_the_conv_losses_on_a_layer); the sweep's error is not above that
    of rounding u* to the nearest level of the same grid."""
    from efficientq_amd import gptq
    gen = torch.Generator().manual_seed(11)
    c, S, N = 8, 12, 2
    conv = gptq.GPTQConvHIP(c, c, 3, 1, 1, 1, 1, True, q_weight=True, qlvl=levels, q_act=True, qlvl_act=4,
                            lwq_channel_wise=channel_wise)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (2.0 / (c * 27)) ** 0.5)
        conv.bias.copy_(torch.randn(c, generator=gen) * 0.1)
    x_fp = torch.relu(torch.randn(N, c, S, S, S, generator=gen))
    y = torch.nn.functional.conv3d(x_fp, conv.weight.data, conv.bias.data, 1, 1)
    x = torch.relu(x_fp + 0.05 * torch.randn(x_fp.shape, generator=gen))
    conv.output_fp, conv.name, conv.layer_loss = y.to(DEV), "l", []
    conv.to(DEV)
    seen = {}
    run = conv._gptq_run
    conv._gptq_run = lambda c_, A0, B0, eta: seen.setdefault("fit", (A0, eta, run(c_, A0, B0, eta)))[2]
    conv.set_quantizing()
    with torch.no_grad():
        conv(x.to(DEV))
    tr = conv.last_trace
    assert tr["method"] == "gptq" and tr["loss_history"] == [] and len(tr["w_iters"]) == 1 and tr["w_iters"][0] >= 1
    w, a_w = conv.weight.data.clone(), conv.alpha_w.data.clone()
    assert tuple(a_w.shape) == ((c, 1, 1, 1) if channel_wise else ())
    # layer_loss against fp64
    xq = conv._quantize_act(x.to(DEV)).double().cpu()
    out = torch.nn.functional.conv3d(xq, w.double().cpu(), conv.bias.data.double().cpu(), 1, 1)
    want = float(((out - y.double()) ** 2).mean())
    got = float(conv.layer_loss[0].split(":")[1])
    print(f"L = {levels}, channel_wise = {channel_wise}: layer_loss {got:.9g}, fp64 {want:.9g}, rel {abs(got / want - 1):.3g}")
    assert abs(got - want) <= 2e-6 * want and abs(tr["layer_loss"] - got) == 0.0
    # gptq_err against round-to-nearest of u* (the bias left at its optimum)
    A0, eta, fit = seen["fit"]
    H = A0.double().cpu().numpy() + eta * np.eye(A0.shape[0])
    u_w = fit.keep[1].double().cpu().numpy()
    a = np.asarray(tr["alpha_w"], dtype=np.float64).reshape(-1, 1)
    dq = np.zeros((c, A0.shape[0]))
    dq[:, :-1] = a * gptq.disc64(u_w, a, levels)[0] - u_w
    rtn = float(np.einsum("ri,ij,rj->", dq, H, dq))
    print(f"   gptq_err {tr['gptq_err']:.6g}, round-to-nearest {rtn:.6g}, ratio {tr['gptq_err'] / rtn:.3f}")
    assert 0.0 < tr["gptq_err"] <= rtn
    # the round trip through the stored ids
    conv.store_int_weight()
    assert conv.weight.data.dtype == torch.uint8 and int(conv.weight.data.max()) <= levels - 1
    conv.weight.data = conv.weight.data.to(DEV)
    conv.restore_fp_weight()
    assert torch.equal(conv.weight.data, w)


def test_ptq_mission_with_qconv_gptq(tmp_path):
    from efficientq_amd import entrance
    snap = str(tmp_path / "snap")
    entrance.main(["ptq", "--task", "lits", "--qconv", "gptq", "--qlvl_w", "4", "--qlvl_a", "4", "--q_first", "256,-1",
                   "--q_last", "256,-1", "--width", "8,16,8", "--depth", "1,1,1", "--init_stride", "1", "--nMod", "1",
                   "--nClass", "3", "--blk", "mid", "--ds", "simple", "--hetero_dim", "--drop_rate", "0.5",
                   "--lwq_batchsz", "2", "--lwq_patchsz", "16,16,16", "--snap_dir", snap, "--synthetic", "--vs_fp"])
    for f in ("layer_loss.txt", "state_in_fp.pkl", "state_in_int8.pkl", "state_in_int8_compress.npz",
              os.path.join("ptq", "agreement.csv")):
        assert os.path.exists(os.path.join(snap, f)), f
    w = torch.load(os.path.join(snap, "state_in_int8.pkl"))["state_dict"]["u_blocks.UResBlock1.Layer1.block1.conv.weight"]
    assert w.dtype == torch.uint8 and int(w.max()) <= 3
    assert len(open(os.path.join(snap, "layer_loss.txt")).read().strip().split("\n")) == 10
