"""Pins the CPU oracle (oracle/effq_oracle.py) to outputs of the real reference
(fixtures written by tests/golden/make_goldens.py).  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import effq_oracle as O

T = torch.from_numpy
pytestmark = pytest.mark.usefixtures("golden_threads")     # the goldens' CPU thread count (conftest.py)


def test_g1_discretize_bit_exact(gold):
    g = gold("g1_discretize.npz")
    for L in (4, 16, 256):
        for tag, lo, hi in (("w", -1, 1), ("a", 0, 1)):
            v = T(g[f"L{L}_{tag}_in"])
            assert torch.equal(O.discretize(v, L, lo, hi), T(g[f"L{L}_{tag}_q32"]))
            assert torch.equal(O.discretize(v.double(), L, lo, hi), T(g[f"L{L}_{tag}_q64"]))
            alpha = torch.tensor(0.7341)
            assert torch.equal(O.discretize(v / alpha, L, lo, hi) * alpha, T(g[f"L{L}_{tag}_qdq32"]))


def test_g2_fit_scale(gold):
    g = gold("g2_project.npz")
    act, wgt = T(g["act"]), T(g["wgt"])
    for L in (4, 16, 256):
        fa = O.fit_scale(act, L, 0, 1)
        assert fa.alpha == float(g[f"act_L{L}_alpha"])
        assert fa.iters == int(g[f"act_L{L}_iters"])
        assert torch.equal(torch.round(fa.b * (L - 1)).to(torch.uint8), T(g[f"act_L{L}_idx"]))
        fw = O.fit_scale(wgt, L, -1, 1)
        assert fw.alpha == float(g[f"wgt_L{L}_alpha"])
        assert fw.iters == int(g[f"wgt_L{L}_iters"])
        assert torch.equal(torch.round((fw.b + 1) * (L - 1) / 2).to(torch.uint8), T(g[f"wgt_L{L}_idx"]))


def test_fit_scale_raises_on_cap():
    # alternating two-cycle cannot be forced cheaply; cap=100*L is hit with tol=0
    v = torch.randn(257)
    with pytest.raises(RuntimeWarning):
        O.fit_scale(v, 4, -1, 1, tol=-1.0)


CASES = [("k3s1p1", 3, 1, 1), ("k3s221p1", 3, (2, 2, 1), 1), ("k1s1p0", 1, 1, 0),
         ("k3s1p1_nobias_noatt", 3, 1, 1)]


@pytest.mark.parametrize("tag,k,s,p", CASES)
def test_g3_g4_gram_and_solve(gold, tag, k, s, p):
    g = gold("g3g4_gram_solve.npz")
    x, y, w = T(g[f"{tag}_x"]), T(g[f"{tag}_y"]), T(g[f"{tag}_w"])
    b = T(g[f"{tag}_b"]) if f"{tag}_b" in g else None
    att = T(g[f"{tag}_att"]) if f"{tag}_att" in g else None
    ps = O.ProxSystem(x, y, (k, k, k), s, p, w.clone(), b.clone() if b is not None else None, att)
    assert torch.equal(ps.A0, T(g[f"{tag}_A0"]))
    assert torch.equal(ps.B0, T(g[f"{tag}_B0"]))
    ws, bs = ps.solve(7.5, 1.3, T(g[f"{tag}_G"]))
    assert torch.equal(ws, T(g[f"{tag}_wstar"]))
    if b is not None:
        assert torch.equal(bs, T(g[f"{tag}_bstar"]))


def test_patch_matrix_is_conv(gold):
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 6, 7, 5, generator=gen)
    w = torch.randn(4, 3, 3, 3, 3, generator=gen)
    cols = torch.from_numpy(O.patch_matrix(x.numpy(), (3, 3, 3), (2, 1, 1), (1, 1, 1)))
    ref = F.conv3d(x, w, None, (2, 1, 1), 1)
    got = (w.reshape(4, -1) @ cols).reshape(4, 2, *ref.shape[2:]).transpose(0, 1)
    assert torch.allclose(got, ref, atol=1e-4)


def test_g7_bn_fold(gold):
    g = gold("g7_bnfold.npz")
    w2, b2 = O.fold_bn_params(T(g["w"]), None, T(g["gamma"]), T(g["beta"]), T(g["mean"]), T(g["var"]),
                              float(g["eps"]))
    assert torch.equal(w2, T(g["w_fold"]))
    assert torch.equal(b2, T(g["b_fold"]))
    y = F.conv3d(torch.relu(T(g["x"])), w2, b2, 1, 1)
    assert torch.equal(y, T(g["y_after"]))
    assert torch.allclose(y, T(g["y_before"]), atol=1e-5)


@pytest.mark.parametrize("task", ["lits", "brats"])
def test_g8_attention_masks(gold, task):
    g = gold("g8_attmask.npz")
    for key, st in ((f"{task}_s1", 1), (f"{task}_s2", (2, 2, 2)), (f"{task}_s221", (2, 2, 1))):
        logits, data = T(g[f"{key}_logits"]), T(g[f"{key}_data"])
        ones = torch.ones_like(data[:, 0]).bool()
        body = (data[:, 0] != 0).bool() if task == "brats" else ones
        wmap, nums = O.class_weights(logits[-1], ones, task)
        assert nums == g[f"{key}_nums"].tolist()
        assert [wmap[i] for i in range(len(wmap))] == g[f"{key}_wvals"].tolist()
        pyr = O.mask_pyramid(logits[-1], body, wmap, st, 3, task)
        for i, m in enumerate(pyr):
            assert torch.equal(m, T(g[f"{key}_pyr{i}"]).float())


def test_g9_int_weight_roundtrip(gold):
    g = gold("g9_intweight.npz")
    for L in (4, 16, 256):
        q, a = T(g[f"L{L}_q"]), T(g[f"L{L}_alpha"])
        idx = O.weight_to_levels(q, a, L)
        assert torch.equal(idx, T(g[f"L{L}_int"]))
        assert torch.equal(O.levels_to_weight(idx, a, L), T(g[f"L{L}_restored"]))


def _g5_case(g, tag):
    c1, c2, k, pad, N, S, L_w, L_a, q_act, with_mask = [int(v) for v in g[f"{tag}_meta"]]
    stride = tuple(int(v) for v in g[f"{tag}_stride"])
    x, y, w = T(g[f"{tag}_x"]).clone(), T(g[f"{tag}_y"]).clone(), T(g[f"{tag}_w_in"]).clone()
    b = T(g[f"{tag}_b_in"]).clone()
    pyr = None
    if with_mask:
        pyr = [torch.ones(N, *[d // 2 for d in y.shape[2:]]), T(g[f"{tag}_mask_full"]).clone()]
    return dict(x=x, y_fp=y, weight=w, bias=b, stride=stride, padding=pad, qlvl_w=L_w, qlvl_act=L_a,
                q_act=bool(q_act), mask_pyramid=pyr)


@pytest.mark.parametrize("tag", ["L4", "L16", "first", "k1"])
def test_g5_layer_calibration_bit_exact(gold, tag):
    g = gold("g5_layer_ptq.npz")
    kw = _g5_case(g, tag)
    res = O.calibrate_layer(**kw)
    assert np.array_equal(np.array(res.loss_history), g[f"{tag}_loss_hist"])
    assert np.array_equal(np.array(res.alpha_w_history), g[f"{tag}_aw_hist"])
    assert torch.equal(res.weight, T(g[f"{tag}_weight"]))
    assert torch.equal(res.bias, T(g[f"{tag}_bias"]))
    assert np.float32(res.alpha_w) == g[f"{tag}_alpha_w"]
    if kw["q_act"]:
        assert np.float32(res.alpha_act) == g[f"{tag}_alpha_act"]
    assert res.layer_loss == float(g[f"{tag}_layer_loss"])
    # the quantised forward that feeds the next layer (PTQConv.py:163-167)
    fwd = O.quantized_forward(kw["x"], res.weight, res.bias, torch.tensor(np.float32(res.alpha_act or 1.0)),
                              kw["qlvl_act"], kw["q_act"], kw["stride"], kw["padding"])
    assert torch.equal(fwd, T(g[f"{tag}_fwd_q"]))


@pytest.mark.parametrize("tag", ["c32", "c64"])
@pytest.mark.parametrize("nt", [8, 1])
def test_g5b_wide_layer_bit_exact_per_thread_count(gold, tag, nt):
    """The reference calibrated the SAME 32->32 / 64->64 layer with 1 and with 8 BLAS threads (make_goldens.g5b);
    the oracle reproduces each run bit for bit at the matching thread count, and the two runs differ from each
    other (the reference's own reproducibility floor, stored as <tag>_spread_*)."""
    g = gold("g5b_wide_layers.npz")
    kw = _g5_case(g, tag)
    kw["mask_pyramid"][1] = kw["mask_pyramid"][1].float()
    before = torch.get_num_threads()
    torch.set_num_threads(nt)
    try:
        res = O.calibrate_layer(**kw)
    finally:
        torch.set_num_threads(before)
    assert np.array_equal(np.array(res.loss_history), g[f"{tag}_t{nt}_loss_hist"])
    assert torch.equal(res.weight, T(g[f"{tag}_t{nt}_weight"]))
    assert torch.equal(res.bias, T(g[f"{tag}_t{nt}_bias"]))
    assert res.layer_loss == float(g[f"{tag}_t{nt}_layer_loss"])
    other = 1 if nt == 8 else 8
    assert not np.array_equal(np.array(res.loss_history), g[f"{tag}_t{other}_loss_hist"])


@pytest.mark.parametrize("tag", ["c32", "c64"])
def test_g5d_fp64_anchor_mode_of_the_oracle(gold, tag):
    """oracle.calibrate_layer(dtype=float64) is the anchor of the wide-layer parity tests.  Switched OFF (fp32) the same
    function reproduces the reference's first proximal solve and first losses bit for bit at the matching thread count
    (make_goldens.g5d stores them from the real reference); switched ON it reproduces the stored anchor, which sits
    <= 1.5e-5 from both reference runs in w*_0 and keeps every iteration-0 level id of the 8-thread run."""
    g, ga = gold("g5b_wide_layers.npz"), gold("g5d_wide_fp64_anchor.npz")
    kw = _g5_case(g, tag)
    kw["mask_pyramid"][1] = kw["mask_pyramid"][1].float()
    before = torch.get_num_threads()
    for nt in (8, 1):
        torch.set_num_threads(nt)
        try:
            res = O.calibrate_layer(iters=8, **kw)
        finally:
            torch.set_num_threads(before)
        assert np.array_equal(np.array(res.loss_history), ga[f"{tag}_t{nt}_loss8"])
        assert torch.equal(res.wstar0, T(ga[f"{tag}_t{nt}_wstar0"])) and torch.equal(res.bstar0, T(ga[f"{tag}_t{nt}_bstar0"]))
    a = O.calibrate_layer(iters=8, dtype=torch.float64, **kw)
    assert a.wstar0.dtype == torch.float64
    assert np.allclose(np.array(a.loss_history), ga[f"{tag}_f64_loss_hist"][:8], rtol=1e-9, atol=0)
    assert torch.allclose(a.wstar0.float(), T(ga[f"{tag}_f64_wstar0"]), rtol=0, atol=1e-7)
    w64 = a.wstar0
    for nt in (1, 8):
        d = ((T(ga[f"{tag}_t{nt}_wstar0"]).double() - w64).norm() / w64.norm()).item()
        assert d <= 1.5e-5, d
    assert int((T(ga[f"{tag}_t8_G0idx"]) != T(ga[f"{tag}_f64_G0idx"])).sum()) == 0
    assert int((T(ga[f"{tag}_t1_G0idx"]) != T(ga[f"{tag}_f64_G0idx"])).sum()) <= 1


def test_g5b_reference_self_spread_is_what_the_fixture_says(gold):
    """Recompute the stored spread from the stored runs: reference-vs-reference (1 vs 8 threads) sits at ~3 % output
    rel-MSE and 5-10 % index mismatch on these layers, i.e. north_star's 1e-3 output bar is not attainable by the
    reference against itself at >= 32 channels."""
    g = gold("g5b_wide_layers.npz")
    for tag in ("c32", "c64"):
        a, b = T(g[f"{tag}_t1_fwd_q"]), T(g[f"{tag}_t8_fwd_q"])
        rel = (((a - b) ** 2).mean() / (b ** 2).mean()).item()
        assert abs(rel - float(g[f"{tag}_spread_out_rel_mse"])) <= 1e-6
        assert rel > 1e-2
        ll = abs(float(g[f"{tag}_t1_layer_loss"]) - float(g[f"{tag}_t8_layer_loss"])) / float(g[f"{tag}_t8_layer_loss"])
        assert abs(ll - float(g[f"{tag}_spread_layer_loss"])) <= 1e-9 and 1e-5 < ll < 5e-3
        assert float(g[f"{tag}_spread_idx_mismatch"]) > 0.01
    # the runs agree at first and separate within a handful of iterations (iteration 5 at 32 channels, 3 at 64)
    assert float(g["c32_spread_hist_first5"]) <= 1e-5 and float(g["c64_spread_hist_first5"]) >= 1e-3


@pytest.mark.parametrize("tag,psz,ov", [("a", 6, 2), ("b", (6, 12, 6), (2, 0, 3)), ("c", 7, 3)])
def test_g11_sliding_window_split_and_stitch(gold, tag, psz, ov):
    """Row f1: patch split / stitch of the reference's evaluation loop, bit for bit."""
    g = gold("g11_sliding_window.npz")
    img = torch.from_numpy(g[f"{tag}_img"])
    patches = O.split_patches(img, psz, ov)
    assert len(patches) == int(g[f"{tag}_npatch"])
    assert torch.equal(torch.stack(patches), torch.from_numpy(g[f"{tag}_patches"]))
    preds = [torch.stack([p * 2.0 + 1.0, p.flip(1) - 0.5]) for p in patches]
    assert torch.equal(O.stitch_patches(img, preds, psz, ov), torch.from_numpy(g[f"{tag}_stitched"]))


def test_g11_dice_helpers(gold):
    g = gold("g11_sliding_window.npz")
    logits = torch.from_numpy(g["m_logits"])
    d_l = torch.stack([d.float() for d in O.dice_vs_label(logits, torch.from_numpy(g["m_tgt_lits"]), "lits")])
    d_b = torch.stack([d.float() for d in O.dice_vs_label(logits, torch.from_numpy(g["m_tgt_brats"]), "brats")])
    assert torch.equal(d_l, torch.from_numpy(g["m_dice_lits"]))
    assert torch.equal(d_b, torch.from_numpy(g["m_dice_brats"]))
    empty = O.dice(torch.zeros(4, dtype=torch.bool), torch.zeros(4, dtype=torch.bool)).float()
    assert torch.equal(empty, torch.from_numpy(g["m_dice_empty"]))


def test_g5e_oracle_reproduces_the_reference_on_many_voxels(gold):
    """g5e: ONE 32 -> 32 3^3 layer on V = 32^3 voxels of one volume (V / n = 38: the regime the bench runs in, against
    V / n = 4 of g5b).  The tensors are rebuilt from the seed (tests/golden_inputs.py; the FP target is exact in fp32 by
    construction) and must match the generator's checksums; the oracle then reproduces the reference's 8-thread run bit
    for bit: 200 losses, final weights, layer_loss."""
    from tests import golden_inputs as GI
    g = gold("g5e_wide_layer_many_voxels.npz")
    tag = "s32"
    S = GI.G5E_CASES[tag]["S"]
    inp = GI.wide_layer_inputs(S, int(g[f"{tag}_seed"]))
    for k in ("w", "b", "x", "y", "mask"):
        assert torch.equal(GI.checksums(inp[k]), T(g[f"{tag}_chk_{k}"])), k
    assert torch.equal(inp["x"][:, ::8, ::8, ::8, ::8], T(g[f"{tag}_x_sub"]))
    assert torch.equal(inp["y"][:, ::8, ::8, ::8, ::8], T(g[f"{tag}_y_sub"]))
    y64 = F.conv3d(inp["x_fp"].double(), inp["w"].double(), inp["b"].double(), 1, 1)
    assert torch.equal(inp["y"].double(), y64)                       # exact: no rounding anywhere in the FP forward
    pyr = [torch.ones(1, S // 2, S // 2, S // 2), inp["mask"]]
    r = O.calibrate_layer(inp["x"], inp["y"], inp["w"], inp["b"], 1, 1, qlvl_w=4, qlvl_act=4, mask_pyramid=pyr)
    assert np.array_equal(np.array(r.loss_history), g[f"{tag}_t8_loss_hist"])
    assert r.layer_loss == float(g[f"{tag}_t8_layer_loss"])
    assert torch.equal(r.weight, T(g[f"{tag}_t8_weight"]))
    assert torch.equal(r.wstar0, T(g[f"{tag}_t8_wstar0"]))


def test_g5e_reference_does_not_agree_with_itself_on_many_voxels_either(gold):
    """What the g5e fixture establishes (VERDICT r3 expected the opposite): with V >> n the reference's runs with 1 and
    with 8 BLAS threads still separate within the first iterations and end 3 - 4 % of the weight ids and 2 % output
    rel-MSE apart - the same distances as on the 12^3 layers of g5b - and even the plateau VALUE (layer_loss) differs by
    8e-4 (32^3) and 3.5e-3 (48^3: north_star's 1e-3 is missed by the reference against itself).  The discrete ADMM
    trajectory amplifies a single flipped weight whatever the conditioning of the system."""
    g = gold("g5e_wide_layer_many_voxels.npz")
    for tag in ("s32", "s48"):
        a, b = g[f"{tag}_t1_loss_hist"], g[f"{tag}_t8_loss_hist"]
        wa, wb = T(g[f"{tag}_t1_weight"]), T(g[f"{tag}_t8_weight"])
        lv = lambda t: torch.round((t / t.abs().max() + 1) * 1.5)
        idx = (lv(wa) != lv(wb)).float().mean().item()
        assert abs(idx - float(g[f"{tag}_spread_idx_mismatch"])) < 1e-12
        assert 0.02 < idx < 0.05
        assert 1e-2 < float(g[f"{tag}_spread_out_rel_mse"]) < 5e-2
        assert 5e-4 < float(g[f"{tag}_spread_layer_loss"]) < 5e-3
        assert np.max(np.abs(a - b) / b) > 0.1                       # the transients differ by > 10 % somewhere
        # and both runs leave the fp64 trajectory within a few iterations as well
        f = g[f"{tag}_f64_loss_hist"]
        assert np.max(np.abs(b[:30] - f[:30]) / f[:30]) > 1e-3 and np.max(np.abs(a[:30] - f[:30]) / f[:30]) > 1e-3
