"""The conv kernels at every geometry their planners accept, against fp64.

The other conv tests run the shipped nets' geometry: cubic kernels of extent 1 or 3, padding k // 2 on every axis, strides 1,
2 and (2, 2, 1).  make_plan (conv3d.hip) takes any extent 1..7, stride and padding per axis, i8_plan any padding, i8s_plan any
geometry of at most 27 taps and K <= 256.  The cases here cover what is accepted and never run: the slab and LDS branches of
the generic tiled kernel, kernels that are not cubic, padding 0, per-axis padding, padding >= k, k_conv3d_c4 (the 4 -> 32
first conv at an anisotropic stride), every i8 kernel off padding 1, and the refusals.

Every case names the plan class it was chosen for and asserts it through effq_conv_plan_query / effq_conv_i8_plan_query /
effq_conv_i8s_plan_query before it runs (tests/test_host_cpu.py asserts the same table without a device), so a retuned
planner fails the case instead of silently moving it to another kernel.

Runs on a real MI355X only (-m gpu); the tables and helpers import without a device."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_tiles_gpu import (_check_poisoned, _close, _ncdhw, _ndhwc, _out_dims, _poison, _sums_vs_fp64,
                                       _triple)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U32 = 2.0 ** -24          # unit roundoff of fp32


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_ops(DEV)


# ------------------------------------------------------------------ the comparison
def value_report(got, ref, S, K):
    """The two value bounds of an fp32 conv output `got` against its fp64 reference `ref` (both fp64 tensors).

    max-norm: the project's max |got - ref| <= 1e-5 max |ref|.

    elementwise: |got - ref| <= (K + 2) 2^-24 S with S = conv3d(|x|, |w|) + |b| and K = C1 * taps.  An output is a K-term
    fp32 dot product followed by the bias add.  Whatever the order of the additions, and whether a product is rounded on its
    own or fused into the addition, every term passes through at most K roundings of the dot product and one of the bias add,
    each of relative size u = 2^-24, so |got - exact| <= ((1 + u)^(K + 1) - 1) S.  (1 + u)^n - 1 <= n u + (n u)^2 / 2 * e^(n u)
    and the second term stays below u while n^2 u <= 1.9, i.e. n = K + 1 <= 5600: then ((1 + u)^(K + 1) - 1) <= (K + 2) u.
    Padded channels and padded taps add exact zeros.  The fp64 reference itself is off by K 2^-53 S, nothing at this scale.

    Returns (max-norm holds, elementwise holds, largest |err| / bound over the outputs with S > 0)."""
    assert K + 1 <= 5600, "the first-order bound needs (K + 1)^2 2^-24 <= 1.9"
    err = (got - ref).abs()
    maxnorm_ok = err.max().item() <= 1e-5 * ref.abs().max().item()
    bound = (K + 2) * U32 * S
    elem_ok = bool((err <= bound).all())
    pos = S > 0
    worst = (err[pos] / bound[pos]).max().item() if bool(pos.any()) else 0.0
    return maxnorm_ok, elem_ok, worst


def check_values(got, ref, S, K, what=""):
    maxnorm_ok, elem_ok, worst = value_report(got, ref, S, K)
    assert maxnorm_ok, f"{what}: max-norm bound missed"
    assert elem_ok, f"{what}: elementwise bound missed, worst |err| / bound = {worst:.3g}"


def check_padding_only(out_ndhwc, cover, bias):
    """Outputs whose receptive field holds no input voxel equal the bias bit for bit (+0 without one).  Returns how many
    voxels that is."""
    m = cover == 0                                               # [OD][OH][OW]
    if not bool(m.any()):
        return 0
    vals = out_ndhwc[:, m, :].contiguous()                       # [N][voxels][C2]
    want = torch.zeros_like(vals) if bias is None else bias.float().view(1, 1, -1).expand_as(vals).contiguous()
    assert torch.equal(vals.view(torch.int32), want.view(torch.int32)), "a padding-only output is not the bias exactly"
    return int(m.sum())


def _cover(sp, k, s, p):
    """Input voxels under each output's kernel window, [OD][OH][OW]."""
    one = torch.ones(1, 1, *sp, dtype=torch.float64)
    return F.conv3d(one, torch.ones(1, 1, *_triple(k), dtype=torch.float64), None, s, p)[0, 0].round().long()


# ------------------------------------------------------------------ f32: the tiled kernels
# id: (c1, c2, k, stride, pad, input spatial, plan class).  N = 2 throughout.  The class holds the fields of
# effq_conv_plan_query the case was chosen for; big_lds: more than 64 KiB of LDS (raise_lds_limit); nh4: halo 16-byte
# loads per slab (3072 = every prefetch register of every thread live).
F32_TILED = {
    "k5_cslab16_two_slabs_nh4_at_the_bound": (32, 32, 5, 1, 2, (9, 9, 17), dict(fast=False, cslab=16, nslab=2, nh4=3072, big_lds=False)),
    "k7_cslab8_big_lds_two_slabs": (16, 40, 7, 1, 3, (8, 9, 12), dict(fast=False, cslab=8, nslab=2, big_lds=True, grid_y=2)),
    "k7_c1_1_big_lds_scalar_loads": (1, 32, 7, 1, 3, (8, 9, 12), dict(fast=False, cslab=8, nslab=1, big_lds=True)),
    "k3_s2_cslab8_big_lds_four_slabs": (32, 64, 3, 2, 1, (17, 15, 33), dict(fast=False, cslab=8, nslab=4, big_lds=True)),
    "k5_s221_4to32_tiled_big_lds": (4, 32, 5, (2, 2, 1), 2, (18, 16, 17), dict(fast=False, cslab=8, nslab=1, big_lds=True)),
    "k1_s2_stride_above_kernel_cslab16": (64, 32, 1, 2, 0, (9, 10, 17), dict(fast=False, cslab=16, nslab=4, big_lds=False)),
    "c2_96_nsub3_nt1": (8, 96, 3, 1, 1, (9, 7, 11), dict(fast=False, nt=1, grid_y=3)),
    "k331_not_cubic": (8, 16, (3, 3, 1), 1, (1, 1, 0), (9, 7, 11), dict(fast=False, cslab=8, nslab=1)),
    "k153_not_cubic": (8, 16, (1, 5, 3), 1, (0, 2, 1), (9, 7, 11), dict(fast=False, cslab=8, nslab=1)),
    "k3_pad0": (8, 16, 3, 1, 0, (10, 9, 13), dict(fast=False, cslab=8)),
    "k3_pad012": (8, 16, 3, 1, (0, 1, 2), (9, 7, 11), dict(fast=False, cslab=8)),
    "k3_pad3_bias_planes": (8, 16, 3, 1, 3, (5, 6, 7), dict(fast=False, cslab=8, padding_only=True)),
    "k3fast_pad0": (32, 32, 3, 1, 0, (10, 10, 18), dict(fast=True, cslab=32, nslab=1)),
    "k3fast_pad2": (32, 32, 3, 1, 2, (6, 6, 14), dict(fast=True, cslab=32, nslab=1)),
}
# the fused activation quantiser: one cslab-16 and one cslab-8 case
F32_FUSED = ("k5_cslab16_two_slabs_nh4_at_the_bound", "k7_cslab8_big_lds_two_slabs")
# geometries make_plan refuses: (c1, c2, k, stride, pad, input spatial)
F32_REFUSED = {
    "k5_s2": (4, 32, 5, 2, 2, (16, 16, 16)),
    "k3_s3": (4, 32, 3, 3, 1, (16, 16, 16)),
    # a stride of 3 under a 1^3 kernel: the staged tile spans 10 x 10 x 22 input voxels, 2/27 of them read (the exact-integer
    # short-K kernel gathers and does serve it: I8S below)
    "k1_s3": (16, 64, 1, 3, 0, (7, 8, 9)),
}
N = 2


def assert_tiled_plan(plan, want):
    """`plan`: conv_plan_query's dict of a call with output or mask; `want`: the class of an F32_TILED case."""
    assert plan["kind"] == 0, plan
    for key in ("fast", "cslab", "nslab", "nt", "grid_y"):
        if key in want:
            assert plan[key] == want[key], (key, plan)
    if "big_lds" in want:
        assert (plan["lds_bytes"] > 64 * 1024) == want["big_lds"], plan
    if "nh4" in want:       # lds_bytes = nhalo * (cslab + 4) floats in the generic kernel
        nhalo = plan["lds_bytes"] // (4 * (plan["cslab"] + 4))
        assert nhalo * plan["cslab"] // 4 == want["nh4"], plan


@functools.lru_cache(maxsize=None)
def _f32_problem(c1, c2, k, s, p, sp, n=N, seed=0):
    """Operands on the host and the fp64 reference, computed once per case.  Weights are continuous random values, so no two
    taps of a kernel are equal and an axis swap cannot hide."""
    kk = _triple(k)
    gen = torch.Generator().manual_seed(1000 + seed + c1 + 7 * c2 + 31 * sum(kk) + sum(sp))
    x = torch.relu(torch.randn(n, c1, *sp, generator=gen))
    w = torch.randn(c2, c1, *kk, generator=gen) * (1.0 / (c1 * math.prod(kk)) ** 0.5)
    b = torch.randn(c2, generator=gen) * 0.1
    out = _out_dims(sp, k, s, p)
    att = torch.tensor([0.25, 1.0, 3.5])[torch.randint(0, 3, (n, *out), generator=gen)]
    noise = torch.randn(n, c2, *out, generator=gen)
    return dict(x=x, w=w, b=b, att=att, noise=noise, K=c1 * math.prod(kk), **_f32_reference(x, w, b, s, p))


def _f32_reference(x, w, b, s, p):
    ref_nb = F.conv3d(x.double(), w.double(), None, s, p)
    S_nb = F.conv3d(x.double().abs(), w.double().abs(), None, s, p)
    bb = b.double().view(1, -1, 1, 1, 1)
    return dict(ref=ref_nb + bb, ref_nb=ref_nb, S=S_nb + bb.abs(), S_nb=S_nb)


def _five_call_forms(ops, geom, pr, cover, xs=None, act=None):
    """The five call forms of test_conv_step_walks_several_tiles_per_workgroup on one problem: output only with and without
    bias, loss with and without the mask, output and loss in one call.  Returns (output with bias, masked-call sums)."""
    x, w, b, att, K = pr["x"], pr["w"], pr["b"], pr["att"], pr["K"]
    ref, ref_nb = pr["ref"], pr["ref_nb"]
    y = (ref + 0.1 * pr["noise"].double()).float()
    xs = _ndhwc(x).to(DEV) if xs is None else xs
    ws, bs, ys, atts = w.to(DEV), b.to(DEV), _ndhwc(y).to(DEV), att.to(DEV)
    kw = {} if act is None else dict(act_alpha=act[0], act_levels=act[1])
    oshape = (ref.shape[0], *ref.shape[2:], ref.shape[1])

    # output only, with bias
    ptr = _poison(oshape)
    out, sq = ops.conv_step(xs, ws, bs, geom, want_out=True, **kw)
    assert sq is None
    _check_poisoned(out, ptr)
    out_b = out.cpu()
    check_values(_ncdhw(out_b).double(), ref, pr["S"], K, "output, bias")
    npad = check_padding_only(out_b, cover, b)
    # output only, without bias
    ptr = _poison(oshape)
    out, _ = ops.conv_step(xs, ws, None, geom, want_out=True, **kw)
    _check_poisoned(out, ptr)
    check_values(_ncdhw(out.cpu()).double(), ref_nb, pr["S_nb"], K, "output, no bias")
    assert check_padding_only(out.cpu(), cover, None) == npad

    # loss with the mask, twice: bit-identical
    _, sq_a = ops.conv_step(xs, ws, bs, geom, ys, atts, **kw)
    la = _sums_vs_fp64(sq_a, ref, y, att)
    _, sq_a2 = ops.conv_step(xs, ws, bs, geom, ys, atts, **kw)
    assert sq_a2.cpu().tolist() == la
    # loss without the mask, twice: bit-identical; the same tiled kernel, so the same summation order
    _, sq_n = ops.conv_step(xs, ws, bs, geom, ys, None, **kw)
    ln = _sums_vs_fp64(sq_n, ref, y, None)
    assert ln[1] == ln[0] == la[0]
    _, sq_n2 = ops.conv_step(xs, ws, bs, geom, ys, None, **kw)
    assert sq_n2.cpu().tolist() == ln
    # bias-free loss
    _, sq_nb = ops.conv_step(xs, ws, None, geom, ys, atts, **kw)
    _sums_vs_fp64(sq_nb, ref_nb, y, att)

    # output and loss in one call: the output-only values and the loss-only sums
    ptr = _poison(oshape)
    out, sq_b = ops.conv_step(xs, ws, bs, geom, ys, atts, want_out=True, **kw)
    _check_poisoned(out, ptr)
    assert torch.equal(out.cpu(), out_b)
    assert sq_b.cpu().tolist() == la
    return out_b, la, npad


@pytest.mark.parametrize("case", list(F32_TILED))
def test_tiled_conv_at_every_accepted_geometry(ops, case):
    """conv3d_quant_calib_step on the tiled kernels, five call forms, against F.conv3d in fp64: max-norm and elementwise
    value bounds, no output left unwritten, padding-only outputs exact, both sums to 1e-5, repeated calls bit-identical."""
    from efficientq_amd.hip_ops import make_geom
    c1, c2, k, s, p, sp, want = F32_TILED[case]
    geom = make_geom((N, c1, *sp), c2, k, s, p)
    assert_tiled_plan(ops.conv_plan(geom), want)
    assert ops.conv_plan(geom, loss_only=True)["kind"] == 0      # no direct kernel takes these: every form is tiled
    pr = _f32_problem(c1, c2, k, s, p, sp)
    _, _, npad = _five_call_forms(ops, geom, pr, _cover(sp, k, s, p))
    assert (npad > 0) == bool(want.get("padding_only", False))


@pytest.mark.parametrize("case", F32_FUSED)
def test_tiled_conv_fused_quantiser_at_new_slab_widths(ops, case):
    """The 4-level activation quantiser fused into the halo staging of the generic kernel at cslab 16 and cslab 8: bit-identical
    to the unfused call on quant_dequant_f32(x), and the five call forms against fp64 on the quantised input."""
    from efficientq_amd.hip_ops import make_geom
    c1, c2, k, s, p, sp, want = F32_TILED[case]
    geom = make_geom((N, c1, *sp), c2, k, s, p)
    assert_tiled_plan(ops.conv_plan(geom), want)
    base = _f32_problem(c1, c2, k, s, p, sp)
    alpha = torch.tensor(0.8123, device=DEV)
    xs = _ndhwc(base["x"]).to(DEV)
    xq = ops.quant_dequant_f32(xs, alpha, 4, 0.0, 1.0)
    pr = dict(base, x=_ncdhw(xq.cpu()), **_f32_reference(_ncdhw(xq.cpu()), base["w"], base["b"], s, p))
    cover = _cover(sp, k, s, p)
    out_f, sums_f, _ = _five_call_forms(ops, geom, pr, cover, xs=xs, act=(alpha, 4))
    out_u, sums_u, _ = _five_call_forms(ops, geom, pr, cover, xs=xq)
    assert torch.equal(out_f, out_u) and sums_f == sums_u


# ------------------------------------------------------------------ f32: the direct kernels (loss only, no mask)
# id: (c1, c2, k, stride, pad, N, input spatial, kernel conv_plan_query must report)
DIRECT = {
    # k_conv3d_c4: 4 -> 32, 3^3 at every stride k_conv3d_c4h has no instance for.  32-voxel wave tiles, 4 waves per workgroup.
    "c4_s221_p1_17tiles_3_idle_waves": (4, 32, 3, (2, 2, 1), 1, 2, (11, 10, 9), "k_conv3d_c4"),       # V = 540
    "c4_s122_p1": (4, 32, 3, (1, 2, 2), 1, 2, (11, 10, 9), "k_conv3d_c4"),                            # V = 550
    "c4_s311_p1": (4, 32, 3, (3, 1, 1), 1, 2, (11, 10, 9), "k_conv3d_c4"),                            # V = 720
    "c4_s221_p0": (4, 32, 3, (2, 2, 1), 0, 2, (11, 10, 9), "k_conv3d_c4"),                            # V = 280
    "c4_s221_p2": (4, 32, 3, (2, 2, 1), 2, 2, (11, 10, 9), "k_conv3d_c4"),                            # V = 924
    "c4_s221_p1_V256_all_waves_busy": (4, 32, 3, (2, 2, 1), 1, 2, (8, 8, 8), "k_conv3d_c4"),          # V = 256
    # the LDS-staged kernels off padding 1; inputs with one tile on the interior path
    "c4h1_p0": (4, 32, 3, 1, 0, 2, (9, 8, 17), "k_conv3d_c4h"),
    "c4h1_p2": (4, 32, 3, 1, 2, 2, (9, 8, 17), "k_conv3d_c4h"),
    "c4h2_p0": (4, 32, 3, 2, 0, 2, (15, 15, 31), "k_conv3d_c4h"),
    "c4h2_p2": (4, 32, 3, 2, 2, 2, (15, 15, 31), "k_conv3d_c4h"),
    "c1h111_p0": (1, 32, 3, 1, 0, 2, (9, 8, 17), "k_conv3d_c1h"),
    "c1h111_p2": (1, 32, 3, 1, 2, 2, (9, 8, 17), "k_conv3d_c1h"),
    "c1h221_p0": (1, 32, 3, (2, 2, 1), 0, 2, (15, 15, 17), "k_conv3d_c1h"),
    "c1h221_p2": (1, 32, 3, (2, 2, 1), 2, 2, (15, 15, 17), "k_conv3d_c1h"),
    "c1h222_p0": (1, 32, 3, 2, 0, 2, (15, 15, 31), "k_conv3d_c1h"),
    "c1h222_p2": (1, 32, 3, 2, 2, 2, (15, 15, 31), "k_conv3d_c1h"),
    # k_conv1_mfma at the two widest inputs, onto one channel and onto four; V = 420 is no multiple of 64 (nor of 16)
    "mfma_128to1": (128, 1, 1, 1, 0, 2, (5, 6, 7), "k_conv1_mfma"),
    "mfma_128to4": (128, 4, 1, 1, 0, 2, (5, 6, 7), "k_conv1_mfma"),
    "mfma_256to1": (256, 1, 1, 1, 0, 2, (5, 6, 7), "k_conv1_mfma"),
    "mfma_256to4": (256, 4, 1, 1, 0, 2, (5, 6, 7), "k_conv1_mfma"),
}


def _staged_interior_tiles(sp, s, p):
    """4 x 4 x 8-voxel output tiles of a 3^3 conv whose whole halo and whole output block lie inside the volumes: the tiles
    k_conv3d_c4h / k_conv3d_c1h fetch through one base address."""
    out = _out_dims(sp, 3, s, p)
    n = 1
    for d, o, ss, pp, t in zip(sp, out, _triple(s), _triple(p), (4, 4, 8)):
        n *= sum(1 for o0 in range(0, o, t) if o0 * ss - pp >= 0 and o0 * ss - pp + (t - 1) * ss + 3 <= d and o0 + t <= o)
    return n


def assert_direct_plan(case, plan):
    c1, c2, k, s, p, n, sp, kernel = DIRECT[case]
    assert plan["kernel"] == kernel, plan
    V = n * math.prod(_out_dims(sp, k, s, p))
    if kernel == "k_conv3d_c4":
        assert plan["ntiles"] == -(-V // 32)
        if "V256" in case:
            assert V % 128 == 0 and plan["grid_x"] * 4 == plan["ntiles"]
        else:
            assert V % 32 != 0                                   # the last wave tile is partial
        if "idle" in case:
            assert plan["grid_x"] * 4 > plan["ntiles"]           # waves without a tile
    elif kernel == "k_conv1_mfma":
        assert V % 64 != 0 and plan["ntiles"] == -(-V // 16)
    else:
        assert 0 < _staged_interior_tiles(sp, s, p) < plan["ntiles"] // n


@pytest.mark.parametrize("case", list(DIRECT))
def test_direct_conv_kernels_off_the_shipped_geometry(ops, case):
    """Loss-only calls without mask on the direct-gather kernels, with and without bias: the sum against fp64 to 1e-5, against
    the tiled kernel's sum of the masked call within the 2e-6 test_conv_step_vs_torch_fp32 allows between the two summation
    orders, bit-identical when repeated."""
    from efficientq_amd.hip_ops import make_geom
    c1, c2, k, s, p, n, sp, _ = DIRECT[case]
    geom = make_geom((n, c1, *sp), c2, k, s, p)
    assert_direct_plan(case, ops.conv_plan(geom, loss_only=True))
    assert ops.conv_plan(geom)["kind"] == 0                      # with a mask the tiled kernel serves it
    pr = _f32_problem(c1, c2, k, s, p, sp, n)
    y = (pr["ref"] + 0.1 * pr["noise"].double()).float()
    xs, ws, ys, atts = _ndhwc(pr["x"]).to(DEV), pr["w"].to(DEV), _ndhwc(y).to(DEV), pr["att"].to(DEV)
    for b, ref in ((pr["b"], pr["ref"]), (None, pr["ref_nb"])):
        bs = None if b is None else b.to(DEV)
        _, sq = ops.conv_step(xs, ws, bs, geom, ys, None)
        got = _sums_vs_fp64(sq, ref, y, None)
        assert got[1] == got[0]
        _, sq2 = ops.conv_step(xs, ws, bs, geom, ys, None)
        assert sq2.cpu().tolist() == got
        _, sq_t = ops.conv_step(xs, ws, bs, geom, ys, atts)
        tiled = _sums_vs_fp64(sq_t, ref, y, pr["att"])
        assert abs(got[0] - tiled[0]) <= 2e-6 * tiled[0], (got, tiled)


# ------------------------------------------------------------------ exact-integer kernels: conv3d_calib_step_i8 / _forward_i8
# id: (c1, c2, output spatial, pad, act levels, weight levels, bias, kernel).  3^3, stride 1: input = output + 2 - 2 pad.
# l2e and i8w need an output their tiles (8 x 4 x 8, 4 x 4 x 8) divide; the others get a ragged one.  Padding 2 cases are large
# enough for one tile on the interior path of the kernels that have one.  512 channels at 4 / 4 levels only.
_PADS = {"p0": 0, "p2": 2, "p012": (0, 1, 2)}
_I8_KERNELS = {
    # kernel: (c1, c2, La, Lw, bias, {pad id: output spatial})
    "l2e": (32, 32, 4, 4, True, dict(p0=(16, 8, 16), p2=(24, 12, 24), p012=(16, 12, 24))),
    "l2": (32, 64, 16, 16, False, dict(p0=(9, 7, 11), p2=(19, 11, 19), p012=(9, 11, 19))),
    "i8<2>": (64, 64, 128, 128, True, dict(p0=(9, 7, 11), p2=(11, 11, 19), p012=(9, 11, 19))),
    "i8w": (64, 64, 4, 4, True, dict(p0=(8, 8, 16), p2=(12, 12, 24), p012=(8, 12, 24))),
    "i8g<4>": (128, 64, 16, 16, False, dict(p0=(9, 7, 11), p2=(11, 11, 19), p012=(9, 11, 19))),
    "i8g<8>": (256, 32, 128, 128, True, dict(p0=(9, 7, 11), p2=(11, 11, 19), p012=(9, 11, 19))),
    "i8g2<16>": (512, 64, 4, 4, True, dict(p0=(5, 7, 11), p2=(7, 11, 19), p012=(5, 11, 19))),
}
I8 = {f"{kern}_{pid}": (c1, c2, outs[pid], _PADS[pid], la, lw, bias, kern)
      for kern, (c1, c2, la, lw, bias, outs) in _I8_KERNELS.items() for pid in _PADS}
# conv3d_quant_forward_i8: the two output-storing kernels at padding 0 and 2, and at padding 3, the smallest at which a 3^3
# kernel has outputs that see only padding (at padding 2 the outermost output plane still reaches input plane 0)
I8_FORWARD = {
    "l2e_p0": I8["l2e_p0"], "l2e_p2": I8["l2e_p2"], "l2e_p3": (32, 32, (16, 8, 16), 3, 4, 4, True, "l2e"),
    "i8w_p0": I8["i8w_p0"], "i8w_p2": I8["i8w_p2"], "i8w_p3": (64, 64, (8, 8, 16), 3, 4, 4, True, "i8w"),
}


def _i8_in(out, pad):
    return tuple(o + 2 - 2 * pp for o, pp in zip(out, _triple(pad)))


@functools.lru_cache(maxsize=None)
def _i8_host_problem(c1, c2, out, pad, la, lw, with_bias, n=N):
    """The operands and the fp64 integer model of test_conv_tiles_gpu._i8_problem, at any padding: conv(level ids, numerators)
    * f32(a_a) f32(a_w) / ((La - 1)(Lw - 1)) + b, exact in fp64 for these sums."""
    sp = _i8_in(out, pad)
    gen = torch.Generator().manual_seed(77 + c1 + 3 * c2 + sum(out) + 5 * sum(_triple(pad)) + la)
    xidx = torch.randint(0, la, (n, *sp, c1), generator=gen, dtype=torch.uint8)
    gq = (2 * torch.randint(0, lw, (c2, c1, 3, 3, 3), generator=gen) - (lw - 1)).to(torch.int8)
    a_act = np.float32(0.8123)
    a_w = np.float32(3.0 / (27 * c1) ** 0.5)            # outputs of order one
    b = torch.randn(c2, generator=gen) * 0.1 if with_bias else None
    y = torch.randn(n, *out, c2, generator=gen)
    att = torch.tensor([0.25, 1.0, 3.5])[torch.randint(0, 3, (n, *out), generator=gen)]
    ref = F.conv3d(xidx.permute(0, 4, 1, 2, 3).double(), gq.double(), None, 1, pad)
    ref = ref * (float(a_act) * float(a_w) / ((la - 1) * (lw - 1)))
    if b is not None:
        ref = ref + b.double().view(1, -1, 1, 1, 1)
    return dict(sp=sp, xidx=xidx, gq=gq, a_act=a_act, a_w=a_w, b=b, y=y, att=att, ref=ref)


def _i8_device(ops, pr):
    st = ops.new_fp_state()
    st[0] = float(pr["a_w"])
    return dict(xidx=pr["xidx"].to(DEV), gq=pr["gq"].to(DEV), b=None if pr["b"] is None else pr["b"].to(DEV),
                y=pr["y"].to(DEV), alpha=torch.tensor(pr["a_act"], device=DEV), st=st)


@pytest.mark.parametrize("case", list(I8))
def test_exact_int_conv_step_off_padding_one(ops, case):
    """conv3d_calib_step_i8 on each of its seven kernels at padding 0, 2 and (0, 1, 2): both sums against the fp64 integer model
    to 1e-6, a repeated call bit-identical."""
    from efficientq_amd.hip_ops import make_geom
    c1, c2, out, pad, la, lw, with_bias, kern = I8[case]
    pr = _i8_host_problem(c1, c2, out, pad, la, lw, with_bias)
    geom = make_geom((N, c1, *pr["sp"]), c2, 3, 1, pad)
    assert geom.out_dims() == out and ops.conv_i8_supported(geom, la, lw)
    assert ops.conv_i8_plan(geom)["kernel"] == kern
    d = _i8_device(ops, pr)
    sq = torch.zeros(2, dtype=torch.float64, device=DEV)
    ops.conv_step_i8(d["xidx"], d["gq"], d["b"], geom, d["y"], d["alpha"], la, d["st"], lw, sq)
    got = _sums_vs_fp64(sq, pr["ref"], _ncdhw(pr["y"]), None, rel=1e-6)
    assert got[1] == got[0]
    sq2 = torch.zeros(2, dtype=torch.float64, device=DEV)
    ops.conv_step_i8(d["xidx"], d["gq"], d["b"], geom, d["y"], d["alpha"], la, d["st"], lw, sq2)
    assert sq2.cpu().tolist() == got


@pytest.mark.parametrize("case", list(I8_FORWARD))
def test_quantised_forward_off_padding_one(ops, case):
    """conv3d_quant_forward_i8 with the mask: every output written, values within 3e-7 of the largest, outputs that see only
    padding equal to the bias bit for bit, both sums to 1e-6, a repeated call bit-identical."""
    from efficientq_amd.hip_ops import make_geom
    c1, c2, out, pad, la, lw, with_bias, kern = I8_FORWARD[case]
    pr = _i8_host_problem(c1, c2, out, pad, la, lw, with_bias)
    geom = make_geom((N, c1, *pr["sp"]), c2, 3, 1, pad)
    assert ops.conv_i8_out_supported(geom, la, lw)
    assert ops.conv_i8_plan(geom, want_out=True)["kernel"] == kern
    d = _i8_device(ops, pr)
    G = (pr["a_w"] * (pr["gq"].float() / (lw - 1))).to(DEV)
    atts = pr["att"].to(DEV)
    ptr = _poison((N, *out, c2))
    o, sq = ops.conv_forward_i8(d["xidx"], G, d["b"], geom, d["y"], atts, d["alpha"], la, d["st"], lw)
    _check_poisoned(o, ptr)
    assert torch.equal(ops._keep_i8[0].reshape(pr["gq"].shape).cpu(), pr["gq"])
    ref = pr["ref"]
    assert (_ncdhw(o).cpu().double() - ref).abs().max().item() <= 3e-7 * ref.abs().max().item()
    npad = check_padding_only(o.cpu(), _cover(pr["sp"], 3, 1, pad), pr["b"])
    assert (npad > 0) == (pad == 3)
    got = _sums_vs_fp64(sq, ref, _ncdhw(pr["y"]), pr["att"], rel=1e-6)
    o2, sq2 = ops.conv_forward_i8(d["xidx"], G, d["b"], geom, d["y"], atts, d["alpha"], la, d["st"], lw)
    assert torch.equal(o2, o) and sq2.cpu().tolist() == got


# ------------------------------------------------------------------ short-K exact-integer kernel: conv3d_calib_step_i8s
# id: (c1, c2, k, stride, pad, La, Lw, input spatial, (NJ, CT, aoff, wmul))
I8S = {
    "4to32_s221_256_256": (4, 32, 3, (2, 2, 1), 1, 256, 256, (11, 10, 9), (4, 1, 128, 2)),
    "4to32_p2_recentred_256_256": (4, 32, 3, 1, 2, 256, 256, (6, 7, 8), (4, 1, 128, 2)),
    # padding 3: outputs that see only padding (-128 in every K slot, numerator exactly 0); not reached at padding 2
    "4to32_p3_padding_only_256_256": (4, 32, 3, 1, 3, 256, 256, (5, 6, 7), (4, 1, 128, 2)),
    "4to32_p012_256_4": (4, 32, 3, 1, (0, 1, 2), 256, 4, (7, 8, 9), (4, 1, 128, 1)),
    "4to32_k133_NJ2_4_256": (4, 32, (1, 3, 3), 1, (0, 1, 1), 4, 256, (6, 7, 9), (2, 1, 0, 2)),
    "16to32_k2_s2_256_256": (16, 32, 2, 2, 0, 256, 256, (8, 8, 8), (4, 1, 128, 2)),
    "16to64_k1_s3_stride_above_kernel_256_4": (16, 64, 1, 3, 0, 256, 4, (7, 8, 9), (1, 2, 128, 1)),
}
# The f32 path refuses this geometry (F32_REFUSED["k1_s3"]).  A 1^3 conv at stride 3 without padding is the 1^3 conv at stride
# 1 of every third voxel - the same dot products of the same operands - so the f32 path runs on the subsampled input instead.
I8S_F32_ON_SUBSAMPLED = ("16to64_k1_s3_stride_above_kernel_256_4",)


def assert_i8s_plan(plan, want, c1, k):
    taps = math.prod(_triple(k))
    assert (plan["NJ"], plan["CT"], plan["aoff"], plan["wmul"]) == want, plan
    assert plan["T"] == taps and plan["K"] == taps * c1, plan


@pytest.mark.parametrize("case", list(I8S))
def test_short_k_exact_int_conv_at_new_geometries(ops, case):
    """conv3d_calib_step_i8s as test_short_k_exact_int_conv_step runs it (operands from the library's own quantiser and
    projection): against the fp64 value of the integer model to 1e-6, against the f32 path on the same operands to 3e-6,
    prepare=True then prepare=False bit-identical."""
    from efficientq_amd import _lib
    from efficientq_amd.hip_ops import make_geom
    c1, c2, k, s, p, La, Lw, sp, want = I8S[case]
    kk = _triple(k)
    gen = torch.Generator().manual_seed(c1 + 7 * c2 + La + 3 * Lw + sum(kk) + sum(sp))
    x = torch.relu(torch.randn(N, *sp, c1, generator=gen) + 0.3).to(DEV)          # NDHWC
    geom = make_geom((N, c1, *sp), c2, k, s, p)
    assert ops.conv_i8s_supported(geom, La, Lw)
    assert_i8s_plan(ops.conv_i8s_plan(geom, La, Lw), want, c1, k)
    a_act, _, st_a = ops.fit_scale(x, La, 0.0, 1.0)
    xq, _, xidx = ops.quant_dequant_f64path(x, st_a, La, 0.0, 1.0, want_idx=True)
    alpha_act = torch.tensor(a_act, dtype=torch.float32, device=DEV)
    wst = (torch.randn(c2, c1, *kk, generator=gen) * 0.05).to(DEV)
    dual, v = torch.zeros_like(wst), torch.empty_like(wst)
    st_w = ops.new_fp_state()
    ops.weight_fixed_point(wst, dual, v, Lw, st_w)
    G = torch.empty_like(wst)
    Gq = torch.empty(wst.shape, dtype=torch.int8, device=DEV)
    ops.admm_project_dual(v, wst, st_w, Lw, G, dual, 1.0, Gq)
    a_w = ops.read_fp_state(st_w)[0]
    num = (2 * Gq.cpu().double() + 1) if Lw > 128 else Gq.cpu().double()       # signed numerators 2 * level - (Lw - 1)
    assert torch.allclose(G.cpu().double(), float(np.float32(a_w)) * num / (Lw - 1), rtol=3e-7, atol=0)
    b = (torch.randn(c2, generator=gen) * 0.1).to(DEV)
    y = torch.randn(N, *geom.out_dims(), c2, generator=gen).to(DEV)
    if case in I8S_F32_ON_SUBSAMPLED:
        assert kk == (1, 1, 1) and _triple(p) == (0, 0, 0)
        with pytest.raises(_lib.EffqError, match="halo"):
            ops.conv_plan(geom, loss_only=True)
        sd, sh, sw = _triple(s)
        xsub = xq[:, ::sd, ::sh, ::sw, :].contiguous()
        _, sq32 = ops.conv_step(xsub, G, b, make_geom((N, c1, *geom.out_dims()), c2, 1, 1, 0), y, None)
    else:
        _, sq32 = ops.conv_step(xq, G, b, geom, y, None)
    sq8 = torch.zeros(2, dtype=torch.float64, device=DEV)
    ops.conv_step_i8s(xidx, Gq, b, geom, y, alpha_act, La, st_w, Lw, sq8, True)
    s32, s8 = sq32.cpu().tolist(), sq8.cpu().tolist()
    out = F.conv3d(xidx.cpu().permute(0, 4, 1, 2, 3).double(), num, None, s, p)
    sc = float(np.float32(a_act)) * float(np.float32(a_w)) / ((La - 1) * (Lw - 1))
    ref = ((out * sc + b.cpu().double().view(1, -1, 1, 1, 1) - _ncdhw(y.cpu()).double()) ** 2).sum().item()
    assert _close(s8[0], ref, 1e-6), (s8, ref)
    assert abs(s8[0] - s32[0]) <= 3e-6 * s32[0], (s8, s32)
    assert s8[1] == s8[0]
    sq8b = torch.zeros(2, dtype=torch.float64, device=DEV)
    ops.conv_step_i8s(xidx, Gq, b, geom, y, alpha_act, La, st_w, Lw, sq8b, False)
    assert sq8b.cpu().tolist() == s8


# ------------------------------------------------------------------ refusals
def _valid_f32_sums(ops):
    """A small valid masked call on the tiled kernel: right sums mean no ticket or workspace state was left behind."""
    from efficientq_amd.hip_ops import make_geom
    c1, c2, k, s, p, sp, _ = F32_TILED["k3_pad012"]
    pr = _f32_problem(c1, c2, k, s, p, sp)
    y = (pr["ref"] + 0.1 * pr["noise"].double()).float()
    _, sq = ops.conv_step(_ndhwc(pr["x"]).to(DEV), pr["w"].to(DEV), pr["b"].to(DEV), make_geom((N, c1, *sp), c2, k, s, p),
                          _ndhwc(y).to(DEV), pr["att"].to(DEV))
    return _sums_vs_fp64(sq, pr["ref"], y, pr["att"])


@pytest.mark.parametrize("case", list(F32_REFUSED))
def test_halo_beyond_lds_is_refused_in_every_call_form(ops, case):
    """k = 5 at stride 2, k = 3 at stride 3 and k = 1 at stride 3: the planner refuses before any launch, in all five call
    forms - the loss-only one of the 4 -> 32, 3^3 layer included, which k_conv3d_c4 could otherwise take - and names the halo."""
    from efficientq_amd import _lib
    from efficientq_amd.hip_ops import make_geom
    c1, c2, k, s, p, sp = F32_REFUSED[case]
    geom = make_geom((N, c1, *sp), c2, k, s, p)
    out = geom.out_dims()
    for lo in (False, True):
        with pytest.raises(_lib.EffqError, match="halo"):
            ops.conv_plan(geom, loss_only=lo)
    first = _valid_f32_sums(ops)
    x = torch.zeros(N, *sp, c1, device=DEV)
    w = torch.zeros(c2, c1, k, k, k, device=DEV)
    b = torch.zeros(c2, device=DEV)
    y = torch.zeros(N, *out, c2, device=DEV)
    att = torch.ones(N, *out, device=DEV)
    forms = [dict(bias=b, want_out=True), dict(bias=None, want_out=True), dict(bias=b, y_ndhwc=y, att=att),
             dict(bias=b, y_ndhwc=y), dict(bias=b, y_ndhwc=y, att=att, want_out=True)]
    for form in forms:
        with pytest.raises(_lib.EffqError, match="halo"):
            ops.conv_step(x, w, form.pop("bias"), geom, **form)
    assert _valid_f32_sums(ops) == first


def test_exact_int_convs_refuse_what_they_cannot_serve(ops):
    """conv_step_i8 on 48 input channels and conv_forward_i8 on a 32 -> 64 layer are refused on the host; a valid call on the
    same HipOps afterwards still gives the right sums."""
    from efficientq_amd import _lib
    from efficientq_amd.hip_ops import make_geom
    case = "l2e_p0"
    c1, c2, out, pad, la, lw, with_bias, _ = I8[case]
    pr = _i8_host_problem(c1, c2, out, pad, la, lw, with_bias)
    geom = make_geom((N, c1, *pr["sp"]), c2, 3, 1, pad)
    d = _i8_device(ops, pr)

    def valid():
        sq = torch.zeros(2, dtype=torch.float64, device=DEV)
        ops.conv_step_i8(d["xidx"], d["gq"], d["b"], geom, d["y"], d["alpha"], la, d["st"], lw, sq)
        return _sums_vs_fp64(sq, pr["ref"], _ncdhw(pr["y"]), None, rel=1e-6)

    first = valid()
    sp = (6, 6, 10)
    sq = torch.zeros(2, dtype=torch.float64, device=DEV)
    g48 = make_geom((N, 48, *sp), 32, 3, 1, 1)
    assert not ops.conv_i8_supported(g48, 4, 4)
    with pytest.raises(_lib.EffqError):
        ops.conv_i8_plan(g48)
    with pytest.raises(_lib.EffqError):
        ops.conv_step_i8(torch.zeros(N, *sp, 48, dtype=torch.uint8, device=DEV),
                         torch.ones(32, 48, 3, 3, 3, dtype=torch.int8, device=DEV), None, g48,
                         torch.zeros(N, *sp, 32, device=DEV), d["alpha"], 4, d["st"], 4, sq)
    g64 = make_geom((N, 32, 8, 4, 8), 64, 3, 1, 1)
    assert ops.conv_i8_supported(g64, 4, 4) and not ops.conv_i8_out_supported(g64, 4, 4)
    assert ops.conv_i8_plan(g64)["kernel"] == "l2"
    with pytest.raises(_lib.EffqError, match="output"):
        ops.conv_i8_plan(g64, want_out=True)
    with pytest.raises(_lib.EffqError, match="output"):
        ops.conv_forward_i8(torch.zeros(N, 8, 4, 8, 32, dtype=torch.uint8, device=DEV),
                            torch.full((64, 32, 3, 3, 3), 0.05, device=DEV), None, g64,
                            torch.zeros(N, 8, 4, 8, 64, device=DEV), None, d["alpha"], 4, d["st"], 4)
    assert float(sq.sum()) == 0.0                                  # nothing was launched into it
    assert valid() == first
