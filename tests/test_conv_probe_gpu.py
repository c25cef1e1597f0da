"""The loss-only conv kernels checked output by output through their sums.

Most conv loss kernels store no output: the suite saw them through sum (out - y)^2 against a random y, where one wrong,
omitted or doubled output disappears in the tolerance.  Here y is built from a bit-exact host model of the kernel's epilogue
(tests/conv_probe_ref.py): with y equal to the model both sums are 0.0 exactly; with y half a unit off on a probe set P they
are 0.25 |P| and 0.25 sum_P att exactly, whatever the order of the additions.  Probe sets: nothing, everything, and one per
bit of each output coordinate (n, od, oh, ow, channel), about 20 launches per case; the planes that fail spell out the
coordinates of a faulty output.  Every integer case asserts equality of both sums, never closeness.

The fp32 kernels have no bit model (the order of their dot products is their own); their probes use the elementwise bound of
test_conv_geometry_gpu.value_report and an offset large enough to stand out of it (see test_f32_loss_only_probes).

Runs on a real MI355X only (-m gpu); tests/test_conv_probe_cpu.py checks the host side without a device."""
import math

import numpy as np
import pytest
import torch

from tests import conv_probe_ref as R
from tests import test_conv_geometry_gpu as G
from tests import test_conv_tiles_gpu as T
from tests.test_conv_geometry_gpu import N, U32, _i8_device, _i8_host_problem

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_worst = {}


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_ops(DEV)


def _record(group, tag, ratio):
    _worst.setdefault(group, {})[tag] = float(ratio)
    print(f"{group} {tag}: error / bound = {ratio:.4g} (worst of the group so far {max(_worst[group].values()):.4g})")


def _up(y):
    return torch.from_numpy(np.ascontiguousarray(y)).to(DEV)


def _step_i8(ops, d, geom, la, lw):
    def launch(y):
        sq = torch.zeros(2, dtype=torch.float64, device=DEV)
        ops.conv_step_i8(d["xidx"], d["gq"], d["b"], geom, _up(y), d["alpha"], la, d["st"], lw, sq)
        return sq.cpu().tolist()
    return launch


def _forward_i8(ops, d, gq, a_w, geom, la, lw, att, o):
    """conv_forward_i8 with the mask: the stored output equals the model bit for bit on every launch."""
    Gw = (a_w * (gq.float() / (lw - 1))).to(DEV)
    atts = att.to(DEV)
    want = torch.from_numpy(o).view(torch.int32)

    def launch(y):
        out, sq = ops.conv_forward_i8(d["xidx"], Gw, d["b"], geom, _up(y), atts, d["alpha"], la, d["st"], lw)
        assert torch.equal(ops._keep_i8[0].reshape(gq.shape).cpu(), gq)
        got = out.cpu().view(torch.int32)
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            raise AssertionError(f"{len(bad)} stored outputs differ from the model in their bits, first at (n, od, oh, ow, c) = "
                                 f"{bad[:4].tolist()}")
        return sq.cpu().tolist()
    return launch


def _step_i8s(ops, pr, geom, la, lw):
    """prepare=True on the first launch of the case, prepare=False afterwards: the cached Su is the one probed."""
    st = ops.new_fp_state()
    st[0] = float(pr["a_w"])
    xidx, gop, b = pr["xidx"].to(DEV), pr["gop"].to(DEV), pr["b"].to(DEV)
    alpha = torch.tensor(pr["a_act"], device=DEV)
    calls = []

    def launch(y, gop_dev=None):
        sq = torch.zeros(2, dtype=torch.float64, device=DEV)
        ops.conv_step_i8s(xidx, gop if gop_dev is None else gop_dev, b, geom, _up(y), alpha, la, st, lw, sq, not calls)
        calls.append(1)
        return sq.cpu().tolist()
    return launch


# ------------------------------------------------------------------ a. the seven tiled exact-integer kernels
@pytest.mark.parametrize("case", [f"{kern}_{pid}" for kern in G._I8_KERNELS for pid in ("p0", "p012")])
def test_exact_int_step_probes(ops, case):
    """conv_step_i8 on each of the seven kernels at the ragged p0 and p012 shapes: the whole probe family, both sums equal to
    0.25 |P| exactly (the call takes no mask: the second sum is the first)."""
    from efficientq_amd.hip_ops import make_geom
    c1, c2, out, pad, la, lw, with_bias, kern = G.I8[case]
    pr = _i8_host_problem(c1, c2, out, pad, la, lw, with_bias)
    geom = make_geom((N, c1, *pr["sp"]), c2, 3, 1, pad)
    assert geom.out_dims() == out and ops.conv_i8_supported(geom, la, lw)
    assert ops.conv_i8_plan(geom)["kernel"] == kern
    o, _ = R.i8_model(pr["xidx"], pr["gq"], pr["b"], pr["a_act"], pr["a_w"], la, lw, pad)
    assert R.run_family(_step_i8(ops, _i8_device(ops, pr), geom, la, lw), o) >= 18


_FORWARD = {**{f"{k}_{pid}": G.I8[f"{k}_{pid}"] for k in ("l2e", "i8w") for pid in ("p0", "p012")},
            "l2e_p3": G.I8_FORWARD["l2e_p3"], "i8w_p3": G.I8_FORWARD["i8w_p3"]}


@pytest.mark.parametrize("case", list(_FORWARD))
def test_quantised_forward_probes(ops, case):
    """conv_forward_i8 (the output-storing l2e and i8w) with the mask at p0, p012 and p3, where outputs see only padding: the
    stored output equals the model bit for bit, the plain sum is 0.25 |P| and the weighted one 0.25 sum_P att, exactly."""
    from efficientq_amd.hip_ops import make_geom
    c1, c2, out, pad, la, lw, with_bias, kern = _FORWARD[case]
    pr = _i8_host_problem(c1, c2, out, pad, la, lw, with_bias)
    geom = make_geom((N, c1, *pr["sp"]), c2, 3, 1, pad)
    assert ops.conv_i8_out_supported(geom, la, lw)
    assert ops.conv_i8_plan(geom, want_out=True)["kernel"] == kern
    o, num = R.i8_model(pr["xidx"], pr["gq"], pr["b"], pr["a_act"], pr["a_w"], la, lw, pad)
    if pad == 3:
        cover = G._cover(pr["sp"], 3, 1, pad).numpy()
        assert (cover == 0).any() and (num[:, cover == 0, :] == 0).all()
    launch = _forward_i8(ops, _i8_device(ops, pr), pr["gq"], pr["a_w"], geom, la, lw, pr["att"], o)
    assert R.run_family(launch, o, pr["att"].numpy()) >= 18


# ------------------------------------------------------------------ b. the short-K kernel
def _i8s_geom(ops, case):
    from efficientq_amd.hip_ops import make_geom
    c1, c2, k, s, p, la, lw, sp, want = R.i8s_case(case)
    geom = make_geom((N, c1, *sp), c2, k, s, p)
    assert ops.conv_i8s_supported(geom, la, lw)
    G.assert_i8s_plan(ops.conv_i8s_plan(geom, la, lw), want, c1, k)
    return geom, la, lw


@pytest.mark.parametrize("case", list(G.I8S) + list(R.I8S_EXTRA))
def test_short_k_probes(ops, case):
    """conv_step_i8s at every geometry of I8S (and at K = 256): the whole family, both sums exact, through the cached Su."""
    geom, la, lw = _i8s_geom(ops, case)
    pr = R.i8s_problem(case)
    assert pr["o"].shape == (N, *geom.out_dims(), geom.C2)
    R.run_family(_step_i8s(ops, pr, geom, la, lw), pr["o"])


# ------------------------------------------------------------------ c. several tiles per workgroup
_TILES_KERNEL = {"l2e_32to32": "l2e", "l2_32to64": "l2", "i8_64to64_ragged": "i8<2>", "i8w_64to64": "i8w",
                 "i8g4_128to128": "i8g<4>", "i8g8_256to128": "i8g<8>", "i8g2_512to256": "i8g2<16>"}


@pytest.mark.parametrize("case", list(T.I8_CASES))
def test_exact_int_step_probes_over_several_tiles_per_workgroup(ops, case):
    """Zero residual and the full set where every workgroup walks several tiles: the persistent walk, the clipped last run,
    the idle workgroups of i8w and the targets prefetched one or two tiles ahead."""
    from efficientq_amd.hip_ops import make_geom
    (c1, c2, n, sp, la, lw), gq, a_w, _, _, _, d = T._i8_problem(ops, case, seed=5 + sum(map(ord, case)))
    geom = make_geom((n, c1, *sp), c2, 3, 1, 1)
    plan = ops.conv_i8_plan(geom)
    assert plan["kernel"] == _TILES_KERNEL[case] and plan["grid_x"] < plan["ntiles"]
    b = None if d["b"] is None else d["b"].cpu()
    o, _ = R.i8_model(d["xidx"].cpu(), gq, b, d["alpha"].item(), a_w, la, lw, 1)
    assert R.run_family(_step_i8(ops, d, geom, la, lw), o, only=("zero", "full")) == 2


# ------------------------------------------------------------------ d. saturated accumulators
@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("kern", list(G._I8_KERNELS))
def test_exact_int_step_with_saturated_accumulators(ops, kern, pattern):
    """Every id at 127 and every numerator at +127 / -127 / a checkerboard of both, at 128 / 128 levels (accepted for every
    kernel, the 512-channel one included, and 129 levels refused: asserted): the largest accumulators the kernels admit,
    27 C1 127^2.  From 64 input channels on that exceeds 2^24; with 32 channels the largest admitted value is 13 935 456
    < 2^24, so for l2e and l2 the case pins the magnitude instead.  Exceeding 2^24 does not make f32(num) round in these three
    patterns - every numerator is 127^2 C1 / 2 times a small count - so a fourth, `odd` (channel 0 one level lower), has odd
    numerators above 2^24 and asserts that the conversion rounds.  Zero residual and the full set."""
    from efficientq_amd.hip_ops import make_geom
    c1, c2, _, _, with_bias, outs = G._I8_KERNELS[kern]
    la = lw = 128
    out, pad = outs["p012"], G._PADS["p012"]
    pr = R.saturated_i8_problem(c1, c2, out, pad, la, lw, with_bias, pattern)
    geom = make_geom((N, c1, *pr["sp"]), c2, 3, 1, pad)
    assert ops.conv_i8_supported(geom, la, lw) and not ops.conv_i8_supported(geom, 129, 128)
    assert ops.conv_i8_plan(geom)["kernel"] == kern
    peak = int(np.abs(pr["num"]).max())
    rounds = bool((pr["num"].astype(np.float32).astype(np.int64) != pr["num"]).any())
    if pattern in ("pos", "neg"):
        assert peak == 27 * c1 * 127 * 127 and (peak > 2 ** 24) == (c1 >= 64)
    elif pattern == "odd":
        assert peak == 27 * 127 * (127 * c1 - 1) and (peak > 2 ** 24) == (c1 >= 64)
        assert rounds == (c1 >= 64)                       # the pattern in which the conversion does round
    else:
        assert peak >= 27 * c1 * 127 * 127 // 4 and pr["num"].min() < 0 < pr["num"].max()
    assert R.run_family(_step_i8(ops, _i8_device(ops, pr), geom, la, lw), pr["o"], only=("zero", "full")) == 2


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("case", R.I8S_SATURATED)
def test_short_k_with_saturated_accumulators(ops, case, pattern):
    """The 256 / 256-level short-K kernel with every id at 255 and every numerator at +-255: |num| = 255^2 x (taps inside) x C1,
    up to K 255^2 = 16 646 400 at K = 256, the longest K i8s_plan takes - just below 2^24, so no admitted input makes this
    kernel's conversion round; the case pins the largest magnitude and the int32 intermediates acc + 128 Ksum."""
    geom, la, lw = _i8s_geom(ops, case)
    assert (la, lw) == (256, 256)
    pr = R.i8s_problem(case, pattern)
    if pattern in ("pos", "neg"):
        K = geom.C1 * geom.KD * geom.KH * geom.KW
        assert int(np.abs(pr["num"]).max()) == K * 255 * 255
    R.run_family(_step_i8s(ops, pr, geom, la, lw), pr["o"], only=("zero", "full"))


# ------------------------------------------------------------------ e. one numerator one level off
# fp32 roundings a squared error passes through before it reaches the fp64 sum, from each kernel's epilogue:
#   epilogue_cells (i8<2>, i8g<4>, i8g<8>, i8g2<16>) and epilogue_masked (l2): f32(d * d), then fp64 additions: 1
#   epilogue_even (l2e: two planes, i8w: one): chains s[r & 3] of 4 * NPL fused d * d + s, then (s0 + s1) + (s2 + s3): 4 NPL + 2
#   k_conv3d_i8s: chains s4[r & 3] of 4 * CT = 4 * C2 / 32 fused terms, then the same three additions: 4 CT + 2
_ROUNDINGS = {"l2e": 10, "l2": 1, "i8<2>": 1, "i8w": 6, "i8g<4>": 1, "i8g<8>": 1, "i8g2<16>": 1}


def _sensitivity(launch_sum, o, o_bumped, roundings, tag):
    """Bound: every d_i^2 >= 0 reaches the sum through at most M fp32 roundings of relative size u = 2^-24 and fp64 additions
    (n 2^-53, nothing here), so |got - sum d_i^2| <= ((1 + u)^M - 1) sum d_i^2 <= (M + 1) u sum d_i^2, with d_i = f32(o'_i - o_i)
    from the two bit models and the squares and their sum taken in fp64."""
    d = (o_bumped - o).astype(np.float64)
    want = float((d * d).sum())
    assert want > 0.0 and int((d != 0).sum()) > 1
    got = launch_sum
    assert got[0] > 0.0 and got[1] == got[0]
    bound = (roundings + 1) * U32 * want
    _record("one-level", tag, abs(got[0] - want) / bound)
    assert abs(got[0] - want) <= bound, (got, want, bound)
    return want


@pytest.mark.parametrize("kern", list(G._I8_KERNELS))
def test_one_level_in_one_tap_is_seen(ops, kern):
    """One numerator of Gq one level (2) off at a single (c2, c1, tap), y at the unmodified model: the sum is positive and
    equals the fp64 value of sum (delta out)^2 to (M + 1) 2^-24 of it, M the kernel's entry in _ROUNDINGS (derivation in
    _sensitivity).  The old comparison - a random y, rel 1e-6 of a sum of 1e5 - cannot see this."""
    from efficientq_amd.hip_ops import make_geom
    c1, c2, out, pad, la, lw, with_bias, _ = G.I8[f"{kern}_p012"]
    pr = _i8_host_problem(c1, c2, out, pad, la, lw, with_bias)
    geom = make_geom((N, c1, *pr["sp"]), c2, 3, 1, pad)
    assert ops.conv_i8_plan(geom)["kernel"] == kern
    o, _ = R.i8_model(pr["xidx"], pr["gq"], pr["b"], pr["a_act"], pr["a_w"], la, lw, pad)
    gq2, step = R.bump_one_numerator(pr["gq"], c2 - 3, c1 - 5, 14, lw)
    assert int((gq2 != pr["gq"]).sum()) == 1 and abs(step) == 2 and int(gq2.abs().max()) <= lw - 1
    o2, _ = R.i8_model(pr["xidx"], gq2, pr["b"], pr["a_act"], pr["a_w"], la, lw, pad)
    d = dict(_i8_device(ops, pr), gq=gq2.to(DEV))
    want = _sensitivity(_step_i8(ops, d, geom, la, lw)(o), o, o2, _ROUNDINGS[kern], kern)
    # for the record: what the comparison against the random y of the problem allows, 1e-6 of its sum
    old = float(((torch.from_numpy(o).double() - pr["y"].double()) ** 2).sum())
    print(f"one-level {kern}: sum (delta out)^2 = {want:.4g}, the tolerance of the comparison with a random y = {1e-6 * old:.4g}")


@pytest.mark.parametrize("case", ["4to32_p2_recentred_256_256", "16to64_k1_s3_stride_above_kernel_256_4"])
def test_one_level_in_one_tap_is_seen_by_the_short_k_kernel(ops, case):
    """The same for conv_step_i8s (one and two column tiles): M = 4 CT + 2."""
    geom, la, lw = _i8s_geom(ops, case)
    pr = R.i8s_problem(case)
    taps = geom.KD * geom.KH * geom.KW
    gop2 = pr["gop"].clone()
    flat = gop2.view(geom.C2, geom.C1, taps)
    lo, hi = (-128, 127) if lw > 128 else (-(lw - 1), lw - 1)
    step = (1 if lw > 128 else 2)
    step = -step if int(flat[geom.C2 - 3, geom.C1 - 2, taps // 2]) + step > hi else step
    flat[geom.C2 - 3, geom.C1 - 2, taps // 2] += step
    assert int(gop2.min()) >= lo and int(gop2.max()) <= hi and int((gop2 != pr["gop"]).sum()) == 1
    c1, c2, k, s, p = R.i8s_case(case)[:5]
    o2, _ = R.i8s_model(pr["xidx"], gop2, pr["b"], pr["a_act"], pr["a_w"], la, lw, s, p)
    launch = _step_i8s(ops, pr, geom, la, lw)
    assert launch(pr["o"]) == [0.0, 0.0]
    ct = -(-geom.C2 // 32)
    _sensitivity(launch(pr["o"], gop2.to(DEV)), pr["o"], o2, 4 * ct + 2, case)


# ------------------------------------------------------------------ f. the fp32 loss-only kernels
# id: (table, case, with the mask)
_F32_PROBES = {
    "k_conv3d_c4": (G.DIRECT, "c4_s221_p1_17tiles_3_idle_waves", False),
    "k_conv3d_c4h": (G.DIRECT, "c4h2_p2", False),
    "k_conv3d_c1h": (G.DIRECT, "c1h221_p2", False),
    "k_conv1_mfma": (G.DIRECT, "mfma_128to4", False),
    "k3fast_pad0": (G.F32_TILED, "k3fast_pad0", True),
    "k3_pad012": (G.F32_TILED, "k3_pad012", True),
}
_F32_ROUNDINGS = 20


def _exact_difference(r, y):
    """double(r) - double(y) with TwoSum's error term asserted zero: the host knows f32(ref_i) - y_i exactly."""
    a, b = r.astype(np.float64), -y.astype(np.float64)
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    assert not err.any()
    return s


@pytest.mark.parametrize("kernel", list(_F32_PROBES))
def test_f32_loss_only_probes(ops, kernel):
    """No bit model exists for the fp32 kernels, so the probes work inside the elementwise bound of value_report:
    |out_i - ref_i| <= (K + 2) u S_i, u = 2^-24.  With r_i = f32(ref_i), |out_i - r_i| <= e_i = (K + 2) u S_i + 2^-25 |ref_i|.

    y_i = r_i outside the probe set P and f32(r_i - delta) inside, delta the smallest power of two >= 4 sum_all e_i (one per
    case); dl_i = r_i - y_i is known exactly on the host (_exact_difference), 0 outside P.  The kernel forms
    d_i = fl(out_i - y_i) = (dl_i + eps_i)(1 + t), |eps_i| <= e_i, |t| <= u, squares and sums.  Every d_i^2 >= 0 passes
    through at most M fp32 roundings on its way into the fp64 sum - the subtraction (twice, being squared), the product or
    the fused chain (at most 16 fused terms in k_conv1_mfma, 4 + 2 in k_conv3d_c4h / _c1h, one in the tiled kernels and none in
    k_conv3d_c4), the product with the mask value - M <= 20 with room to spare, so with rho = (M + 1) u
        | sqerr - sum_P dl_i^2 |  <=  2 sum_P |dl_i| e_i  +  sum_all e_i^2  +  rho sum_all (|dl_i| + e_i)^2
    (cross term, square term, summation rounding), and the same with every term weighted by att_i for sqerr[1].  For the empty
    set this is sqerr <= (1 + rho) sum e_i^2.  Since delta >= 4 sum e_i, the cross term is at most delta^2 / 2: one output
    left out of the sum or counted twice moves it by delta^2, more than twice what rounding may."""
    from efficientq_amd.hip_ops import make_geom
    table, case, with_att = _F32_PROBES[kernel]
    if table is G.DIRECT:
        c1, c2, k, s, p, n, sp, _ = table[case]
        geom = make_geom((n, c1, *sp), c2, k, s, p)
        G.assert_direct_plan(case, ops.conv_plan(geom, loss_only=True))
        assert ops.conv_plan(geom, loss_only=True)["kernel"] == kernel
    else:
        c1, c2, k, s, p, sp, want = table[case]
        n = N
        geom = make_geom((n, c1, *sp), c2, k, s, p)
        G.assert_tiled_plan(ops.conv_plan(geom), want)
        assert ops.conv_plan(geom, loss_only=True)["kind"] == 0
    pr = G._f32_problem(c1, c2, k, s, p, sp, n)
    nd = lambda t: t.permute(0, 2, 3, 4, 1).contiguous().numpy()
    ref, S, K = nd(pr["ref"]), nd(pr["S"]), pr["K"]
    assert K + 1 <= 5600
    r = ref.astype(np.float32)
    e = (K + 2) * U32 * S + 2.0 ** -25 * np.abs(ref)
    delta = 2.0 ** math.ceil(math.log2(4.0 * float(e.sum())))
    assert delta >= 4.0 * e.sum() > delta / 2
    att = pr["att"].numpy().astype(np.float64) if with_att else None
    wgt = np.ones(ref.shape[:4] + (1,)) if att is None else att[..., None]
    xs, ws, bs = T._ndhwc(pr["x"]).to(DEV), pr["w"].to(DEV), pr["b"].to(DEV)
    atts = pr["att"].to(DEV) if with_att else None
    y_off = r - np.float32(delta)
    rho = (_F32_ROUNDINGS + 1) * U32
    fails, notes, worst = [], [], 0.0
    for name, mask in R.probe_sets(r.shape):
        m = np.broadcast_to(mask, r.shape)
        y = np.where(m, y_off, r)
        dl = _exact_difference(r, y)
        assert not dl[~m].any() and (np.abs(dl[m] - delta) <= 2.0 ** -23 * (np.abs(r[m]) + delta)).all()
        _, sq = ops.conv_step(xs, ws, bs, geom, _up(y), atts)
        got = sq.cpu().tolist()
        for j, w in enumerate((np.ones_like(wgt), wgt)):
            want = float((w * dl * dl).sum())
            bound = float((w * (2 * np.abs(dl) * e + e * e + rho * (np.abs(dl) + e) ** 2)).sum())
            ratio = abs(got[j] - want) / bound
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                fails.append((name, [got[j]], [want]))
                notes.append(f"{name} sqerr[{j}]: |got - want| = {ratio:.3g} of the bound {bound:.6g}")
    _record("f32 probes", f"{kernel} delta={delta:g}", worst)
    assert not fails, "\n".join(notes) + "\n" + R.explain(fails, r.shape)
