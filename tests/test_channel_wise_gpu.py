"""Channel mode of the calibrator (lwq_channel_wise: one weight scale per output channel) on a real MI355X (-m gpu): the
per-row fixed point kernel (effq_fixed_point_channels[_proj]) against oracle.fit_scale per row, the product's ptq() in
channel mode against the CPU restatement of tests/channel_backend.py, and the whole ptq mission with the flag."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import effq_oracle as O
from tests import channel_backend as CB
from tests.test_host_cpu import T, _layer_from_gold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd import hip_ops
    return hip_ops.get_ops(torch.device(DEV))


def _rows(c2, nwrow, L, seed):
    """[c2, nwrow] values with row norms spread over 2^0 .. 2^3; row 1 all zero (c2 > 1); row 2 with values ON rounding
    boundaries of its converged and of its start scale, and one ulp either side (c2 > 2)."""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(c2, nwrow, generator=gen) * 0.1
    v *= torch.tensor([2.0 ** (c % 4) for c in range(c2)]).unsqueeze(1)
    if c2 > 1:
        v[1] = 0.0
    if c2 > 2 and nwrow >= 32:
        d = 2.0 / (L - 1)
        bnd = torch.tensor([(k - 0.5) * d - 1.0 for k in range(1, L)], dtype=torch.float64)
        fit = O.fit_scale(v[2], L, -1, 1)
        pts = []
        for a in (fit.alpha, v[2].abs().double().mean().item()):
            p = (bnd * a).float()
            pts += [p, torch.nextafter(p, torch.tensor(10.0)), torch.nextafter(p, torch.tensor(-10.0))]
        pts = torch.cat(pts)[: nwrow // 2]
        v[2, nwrow - pts.numel():] = pts
    return v


def _sample_rows(c2):
    rows = {0, c2 - 1} | ({1, 2} if c2 > 2 else set())
    rows |= set(range(3, c2, max(1, c2 // 6)))
    return sorted(rows)


SHAPES = [(c2, nw) for c2 in (1, 32, 64, 128, 256, 512) for nw in (27, 108, 864, 1728, 3456, 6912, 13824)
          if c2 * nw <= (1 << 22)]


@pytest.mark.parametrize("L", [4, 16, 256])
def test_channel_fixed_point_matches_oracle_per_row(ops, L):
    """alpha_c within 1e-11 of oracle.fit_scale on the row, the same iteration count, the level ids of the epilogue's G
    equal to the oracle's (a flip is allowed only where the oracle's pre-image lies within 1e-9 level units of a
    rounding boundary: the two scales differ in the last bits); the zero row: alpha 0, 0 iterations, G = 0; the epilogue's
    G, dual and Bm equal to the same formulas evaluated in torch with the kernel's alpha_c, bit for bit; two launches
    give the same bits."""
    worst = 0.0
    for k, (c2, nwrow) in enumerate(SHAPES):
        a = _rows(c2, nwrow, L, 100 * L + k)
        gen = torch.Generator().manual_seed(k)
        du0 = torch.randn(c2, nwrow, generator=gen) * 1e-3
        w = (a - du0).contiguous()                 # w* + dual = a up to the fp32 rounding of the sum
        n, ldb = nwrow + 1, (nwrow + 1 + 3) // 4 * 4
        B0 = torch.randn(c2, n, generator=gen)
        W0 = torch.randn(c2, nwrow, generator=gen) * 0.1
        rho, eta, div = 20.0, 3.0, 2.0
        outs = []
        for rep in range(2):
            wd, dd = w.to(DEV), du0.clone().to(DEV)
            v = torch.empty_like(wd)
            G = torch.empty_like(wd)
            Bm = torch.zeros(c2, ldb, device=DEV)
            alpha = torch.empty(c2, dtype=torch.float64, device=DEV)
            iters = torch.empty(c2, dtype=torch.int32, device=DEV)
            err = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.fixed_point_channels(wd, dd, v, L, alpha, iters, err,
                                     proj=dict(G=G, dual_div=div, Bm=Bm, B0=B0.to(DEV), W0=W0.to(DEV), ldb=ldb,
                                               rho_next=rho, eta=eta))
            torch.cuda.synchronize()
            outs.append([t.cpu() for t in (v, G, dd, Bm, alpha, iters, err)])
        for x, y in zip(outs[0], outs[1]):
            assert torch.equal(x, y), (c2, nwrow)
        v, G, dual, Bm, alpha, iters, err = outs[0]
        assert int(err) == 0
        assert torch.equal(v, w + du0)
        for r in _sample_rows(c2):
            if float(v[r].abs().sum()) == 0.0:
                assert float(alpha[r]) == 0.0 and int(iters[r]) == 0 and torch.equal(G[r], torch.zeros(nwrow))
                assert not torch.signbit(G[r]).any()
                continue
            fit = O.fit_scale(v[r], L, -1, 1)
            rel = abs(float(alpha[r]) - fit.alpha) / fit.alpha
            worst = max(worst, rel)
            assert rel <= 1e-11 and int(iters[r]) == fit.iters, (c2, nwrow, r, rel, int(iters[r]), fit.iters)
            ids = O.quant_index(v[r].double() / float(alpha[r]), L, -1, 1)
            ids_ref = O.quant_index(v[r].double() / fit.alpha, L, -1, 1)
            u = (torch.clamp(v[r].double() / fit.alpha, -1, 1) + 1) / (2.0 / (L - 1))
            flips = ids != ids_ref
            assert not flips.any() or float((u[flips] - torch.floor(u[flips]) - 0.5).abs().max()) <= 1e-9, (c2, nwrow, r)
        # the epilogue in torch with the kernel's scales
        a64 = alpha.unsqueeze(1)
        b = O.discretize(v.double() / torch.where(a64 == 0, torch.ones_like(a64), a64), L, -1, 1).float()
        G_t = torch.where(a64 == 0, torch.zeros_like(b), a64.float() * b)
        du_t = ((w - G_t) + du0) / torch.tensor(div, dtype=torch.float32)
        bm_t = (B0[:, :nwrow] + torch.tensor(eta, dtype=torch.float32) * W0) + \
            torch.tensor(rho, dtype=torch.float32) * (G_t - du_t)
        assert torch.equal(G, G_t) and torch.equal(dual, du_t) and torch.equal(Bm[:, :nwrow], bm_t), (c2, nwrow)
    print(f"L={L}: worst alpha rel {worst:.2e} over {len(SHAPES)} shapes")


def test_channel_fixed_point_cap_sets_the_error_flag(ops):
    """A row that needs more than max_iter iterations: flag 2 (the per-tensor path's code), its count = the cap."""
    from efficientq_amd import _lib
    v = _rows(4, 108, 256, 5).to(DEV)
    alpha = torch.empty(4, dtype=torch.float64, device=DEV)
    iters = torch.empty(4, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(ops.lib.effq_fixed_point_channels(v.data_ptr(), None, None, 4, 108, 256, 1e-30, 2, alpha.data_ptr(),
                                                 iters.data_ptr(), err.data_ptr(), ops.stream), "channels")
    torch.cuda.synchronize()
    assert int(err) == 2 and iters.tolist() == [2, 0, 2, 2]


def _to_dev(conv):
    conv.to(DEV)
    conv.output_fp = conv.output_fp.to(DEV)
    if conv.mask_pyramid:
        conv.mask_pyramid = [m.to(DEV) for m in conv.mask_pyramid]
    return conv


def _channel_conv(c1, c2, L_w, L_a, q_act, stride=1, pad=1):
    from efficientq_amd.qconv import EfficientQConvHIP
    return EfficientQConvHIP(c1, c2, 3, stride, pad, 1, 1, True, q_weight=True, qlvl=L_w, q_act=q_act, qlvl_act=L_a,
                             lwq_channel_wise=True, lwq_trace=True)


def _row_ids(w, alpha, L):
    a = alpha.reshape(-1, *([1] * (w.dim() - 1))).double()
    return torch.round((w.double() / torch.where(a == 0, torch.ones_like(a), a) + 1) * (L - 1) / 2)


def _spy_runs(ops_obj):
    runs, orig = [], ops_obj.admm_run

    def spy(*a, **kw):
        runs.append((orig(*a, **kw), a, kw))
        return runs[-1][0]
    ops_obj.admm_run = spy
    return runs


def _iteration0_anchor(run_args, run, L, x_q, y, w_in, b_in, stride, pad, att):
    """alpha_c and ids of iteration 0 against the fp64 anchor (ProxSystem in fp64 on the same quantised input)."""
    (A0, B0, W0, b0, geom, yn), kw = run_args
    sysm = O.ProxSystem(x_q.double(), y.double(), (3, 3, 3), stride, pad, w_in.double(), b_in.double(),
                        att.double() if att is not None else None, dtype=torch.float64)
    ws64, _ = sysm.solve(kw["rho"], kw["eta"], w_in.double())
    a64, _, b64 = CB.fit_rows(ws64, L)
    a_gpu = run.alpha_ring[0].cpu()
    rel = max(abs(float(a_gpu[c]) - a64[c]) / abs(a64[c]) for c in range(len(a64)) if a64[c] != 0)
    G0 = run.G_ring[0].cpu().reshape(ws64.shape)
    ids = _row_ids(G0, a_gpu, L).reshape(len(a64), -1)
    ids64 = torch.round((b64 + 1) * (L - 1) / 2)
    u64 = (torch.clamp(ws64.reshape(len(a64), -1) / torch.tensor(a64, dtype=torch.float64).unsqueeze(1), -1, 1) + 1) \
        * (L - 1) / 2
    flips = ids != ids64
    margin = float((u64[flips] - torch.floor(u64[flips]) - 0.5).abs().max()) if flips.any() else 0.0
    return rel, int(flips.sum()), margin


def test_channel_wise_layer_matches_the_cpu_restatement(gold):
    """The g5 8 -> 8 3^3 layer (2 x 8 x 12^3) in channel mode against the fp32 CPU restatement, at the bars of
    test_layer_calibration_matches_reference: layer_loss within 1e-3, 4-level ids identical, forward rel-MSE <= 1e-3;
    iteration 0 against the fp64 anchor: alpha_c within 1e-5 (measured 1.6e-7: the fp32 prox solve's w* is ~1e-6 from the
    fp64 one and alpha_c is linear in the row, so 1e-9 is out of reach), ids equal except within 1e-4 level units of a
    boundary."""
    import efficientq_amd.qconv as Q
    g = gold("g5_layer_ptq.npz")
    base, x, (L_w, L_a, q_act) = _layer_from_gold(g, "L4")
    conv = _channel_conv(8, 8, L_w, L_a, q_act, tuple(base.stride), base.padding)
    conv.weight.data, conv.bias.data = base.weight.data.clone(), base.bias.data.clone()
    conv.output_fp, conv.name, conv.layer_loss, conv.mask_pyramid = base.output_fp, "layer", [], base.mask_pyramid
    ref = CB.calibrate_layer_channels(x, base.output_fp, base.weight.data, base.bias.data, tuple(base.stride),
                                      base.padding, qlvl_w=L_w, qlvl_act=L_a, q_act=q_act, mask_pyramid=base.mask_pyramid)
    _to_dev(conv)
    opsd = Q.get_ops(torch.device(DEV))
    runs = _spy_runs(opsd)
    try:
        conv.set_quantizing()
        with torch.no_grad():
            out = conv(x.to(DEV)).cpu()
    finally:
        del opsd.admm_run
    tr = conv.last_trace
    assert tr["channel_wise"] and not tr["exact_int"] or tr["gram_loss"]
    got = float(conv.layer_loss[0].split(":")[1])
    assert abs(got - ref.layer_loss) <= 1e-3 * ref.layer_loss, (got, ref.layer_loss)
    w, a = conv.weight.data.cpu(), conv.alpha_w.data.cpu()
    assert CB.rows_on_grid(w, a, L_w)
    assert torch.equal(_row_ids(w, a, L_w), _row_ids(ref.weight, torch.tensor(ref.alpha_w), L_w))
    ref_out = O.quantized_forward(x, ref.weight, ref.bias, torch.tensor(np.float32(ref.alpha_act)), L_a, q_act,
                                  tuple(base.stride), base.padding)
    rel_mse = (((out - ref_out) ** 2).mean() / (ref_out ** 2).mean()).item()
    assert rel_mse <= 1e-3
    rel, flips, margin = _iteration0_anchor((runs[0][1], runs[0][2]), runs[0][0], L_w, ref.qact, base.output_fp,
                                            base.weight.data, base.bias.data, tuple(base.stride), base.padding,
                                            O.pick_mask(base.mask_pyramid, base.output_fp.shape))
    print(f"g5 L4 channel mode: layer_loss {got:.6g} vs {ref.layer_loss:.6g}, out rel-MSE {rel_mse:.2e}, "
          f"iteration 0 vs fp64: alpha rel {rel:.2e}, {flips} id flips (margin {margin:.1e})")
    assert rel <= 1e-5 and (flips == 0 or margin <= 1e-4)


def _wide_conv(S, c=32, seed=3032):
    from tests import golden_inputs as GI
    inp = GI.wide_layer_inputs(S, seed, c, c)
    conv = _channel_conv(c, c, 4, 4, True)
    conv.weight.data, conv.bias.data = inp["w"].clone(), inp["b"].clone()
    conv.output_fp, conv.name, conv.layer_loss = inp["y"], "layer", []
    conv.mask_pyramid = [torch.ones(1, S // 2, S // 2, S // 2), inp["mask"]]
    return conv, inp


def _run_wide(conv, x):
    import efficientq_amd.qconv as Q
    _to_dev(conv)
    opsd = Q.get_ops(torch.device(DEV))
    runs = _spy_runs(opsd)
    try:
        conv.set_quantizing()
        with torch.no_grad():
            out = conv(x.to(DEV)).cpu()
    finally:
        del opsd.admm_run
    torch.cuda.synchronize()
    return out, runs[0]


def test_channel_wise_32_channel_layer_gram_loss_and_conv_loss(gold, monkeypatch):
    """A g5e-style 32 -> 32 3^3 layer on 32^3 voxels (tests/golden_inputs.py, s32) takes loss kind 4 (fp64 Gram system)
    in channel mode: against the fp32 CPU restatement at g5e's bars (layer_loss 6e-3, ids 5 %); with the Gram loss
    switched off it takes kind 0 (f32 conv), and all 200 losses agree with kind 4's within 2e-6; iteration 0 against the
    fp64 anchor at the bars of the 8-channel test (measured: alpha_c 5.5e-7, no id flips)."""
    import efficientq_amd.qconv as Q
    S = 32
    res = {}
    for gl in (True, False):
        monkeypatch.setattr(Q, "GRAM_LOSS_DEFAULT", gl)
        conv, inp = _wide_conv(S)
        out, run = _run_wide(conv, inp["x"])
        tr = dict(conv.last_trace)
        assert tr["channel_wise"] and tr["gram_loss"] == gl
        res[gl] = (np.array(tr["loss_history"]), conv.weight.data.cpu(), conv.alpha_w.data.cpu(),
                   float(conv.layer_loss[0].split(":")[1]), run)
    hg, hc = res[True][0], res[False][0]
    assert np.all(np.abs(hg - hc) <= 2e-6 * hc), np.abs(hg / hc - 1).max()
    conv, inp = _wide_conv(S)
    ref = CB.calibrate_layer_channels(inp["x"], inp["y"], inp["w"], inp["b"], 1, 1, qlvl_w=4, qlvl_act=4, q_act=True,
                                      mask_pyramid=conv.mask_pyramid)
    got = res[True][3]
    assert abs(got - ref.layer_loss) <= 6e-3 * ref.layer_loss, (got, ref.layer_loss)
    w, a = res[True][1], res[True][2]
    assert CB.rows_on_grid(w, a, 4)
    mism = (_row_ids(w, a, 4) != _row_ids(ref.weight, torch.tensor(ref.alpha_w), 4)).float().mean().item()
    assert mism <= 5e-2
    run, args, kw = res[True][4]
    rel, flips, margin = _iteration0_anchor((args, kw), run, 4, ref.qact, inp["y"], inp["w"], inp["b"], 1, 1,
                                            inp["mask"])
    print(f"s32 channel mode: layer_loss {got:.6g} vs {ref.layer_loss:.6g}, ids {mism:.4f}, kind 0 vs 4 max rel "
          f"{np.abs(hg / hc - 1).max():.2e}; iteration 0 vs fp64: alpha rel {rel:.2e}, {flips} flips (margin {margin:.1e})")
    assert rel <= 1e-5 and (flips == 0 or margin <= 1e-4)


def test_channel_wise_128_channel_layer_is_deterministic():
    """128 -> 128 3^3 at V = 32^3 >= 8 n on the default path in channel mode: loss kind 0 (the f32 conv pass: the
    integer paths are off in channel mode), weights on their per-row grids, two runs bit-identical."""
    outs = []
    for _ in range(2):
        conv, inp = _wide_conv(32, c=128, seed=5128)
        out, _ = _run_wide(conv, inp["x"])
        tr = conv.last_trace
        assert tr["channel_wise"] and tr["gram_loss"] is False and not tr["exact_int"]
        outs.append((conv.weight.data.cpu(), conv.alpha_w.data.cpu(), out, tr["loss_history"]))
    assert CB.rows_on_grid(outs[0][0], outs[0][1], 4)
    for x, y in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(x, y)
    assert outs[0][3] == outs[1][3]


def test_ptq_mission_with_the_channel_wise_flag(tmp_path):
    """`entrance ptq --lwq_channel_wise` on a tiny synthetic problem: the artefacts are written, every calibrated layer's
    alpha_w is a per-channel vector and the int8 snapshot holds level ids within the grid."""
    from efficientq_amd import entrance
    snap = str(tmp_path / "snap")
    entrance.main(["ptq", "--task", "lits", "--qconv", "effq", "--qlvl_w", "4", "--qlvl_a", "4", "--q_first", "256,-1",
                   "--q_last", "256,-1", "--width", "8,16,8", "--depth", "1,1,1", "--init_stride", "1", "--nMod", "1",
                   "--nClass", "3", "--blk", "mid", "--ds", "simple", "--hetero_dim", "--drop_rate", "0.5",
                   "--lwq_batchsz", "2", "--lwq_patchsz", "32,32,32", "--synthetic", "--no_test", "--snap_dir", snap,
                   "--lwq_channel_wise"])
    for f in ("layer_loss.txt", "time_cost.txt", "class_voxel_nums.txt", "state_in_fp.pkl", "state_in_int8.pkl",
              "state_in_int8_compress.npz"):
        assert os.path.exists(os.path.join(snap, f)), f
    sd = torch.load(os.path.join(snap, "state_in_int8.pkl"))["state_dict"]
    fp = torch.load(os.path.join(snap, "state_in_fp.pkl"))["state_dict"]
    alphas = {k: v for k, v in sd.items() if k.endswith("alpha_w")}
    assert len(alphas) == 10
    for k, a in alphas.items():
        w = fp[k[:-len("alpha_w")] + "weight"]
        assert tuple(a.shape) == (w.shape[0], 1, 1, 1), k
        L = 256 if int(sd[k[:-len("alpha_w")] + "weight"].max()) > 3 else 4
        assert CB.rows_on_grid(w, a, L, 1e-5), k


@pytest.mark.usefixtures("golden_threads")
def test_whole_tiny_net_in_channel_mode_against_the_cpu_stand_in(gold, monkeypatch):
    """calibrate_model on the tiny BraTS net of g6 in channel mode, on the device and through the CPU stand-in of
    tests/channel_backend.py: per-layer layer_loss within the whole-net bars test_whole_calibration_matches_reference
    uses (12 % per layer, 4 % on the sum)."""
    from efficientq_amd import calibrate as K
    from efficientq_amd import config as Cf
    import efficientq_amd.qconv as Q
    g = gold("g6c_tiny_brats_L4.npz")
    monkeypatch.setattr(K, "ALIAS_FP_TARGETS", False)
    net = dict(Cf.TINY_NET, task="brats", nMod=2, nClass=4, multi_label="brats", init_stride="2,2,2")
    S = int(g["meta"][1])
    losses = {}
    for where in ("cpu", "gpu"):
        args = Cf.make_args(net, 4, 4, lwq_batchsz=2, lwq_channel_wise=True)
        QConv, _, kwQ = Cf.get_conv_class(args)
        model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
        # (the fixture's per-tensor alpha_w scalars are left out: calibration sets them)
        model.load_state_dict({k[4:]: T(g[k]) for k in g.files if k.startswith("sd0/") and not k.endswith("alpha_w")},
                              strict=False)
        model.eval()
        K.search_fold_and_remove_bn(model)
        vols = torch.randn(2, 2, S, S, S, generator=torch.Generator().manual_seed(int(g["vols_seed"])))
        zz = torch.arange(S).float() - (S - 1) / 2
        r = (zz[:, None, None] ** 2 + zz[None, :, None] ** 2 + zz[None, None, :] ** 2).sqrt()
        vols = vols * (r < 0.45 * S).float()
        K.set_name(model)
        with monkeypatch.context() as m:
            if where == "cpu":
                CB.install(m)
            else:
                model.to(DEV)
                vols = vols.to(DEV)
            res = K.calibrate_model(model, vols, "brats", args.init_stride)
        losses[where] = np.array([float(l.split(":")[1]) for l in res["layer_loss"]])
    got, want = losses["gpu"], losses["cpu"]
    print("channel mode whole net, gpu / cpu layer_loss:", np.round(got / want, 4).tolist())
    assert np.all(np.abs(got - want) <= 1.2e-1 * want), (got, want)
    assert abs(got.sum() - want.sum()) <= 4e-2 * want.sum()
