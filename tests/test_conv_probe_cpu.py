"""The host side of tests/test_conv_probe_gpu.py, without a device: the bit models of tests/conv_probe_ref.py against the fp64
integer model, the short-K kernel's re-centring identity, the probe builder against a brute-force float32 evaluation, and the
sign choice on the very inputs the GPU cases use."""
import numpy as np
import pytest
import torch

from tests import conv_probe_ref as R
from tests import test_conv_geometry_gpu as G
from tests import test_conv_tiles_gpu as T

U32 = 2.0 ** -24


def _ndhwc64(ref):
    return ref.permute(0, 2, 3, 4, 1).contiguous().numpy()


@pytest.mark.parametrize("case", list(G.I8) + ["l2e_p3", "i8w_p3"])
def test_i8_model_is_the_fp64_integer_model_to_three_roundings(case):
    """|o - ref| <= 3 * 2^-24 (|scaled num| + |b|): the scale, its product with f32(num) and the bias add round once each;
    f32(num) itself is exact below 2^24, as it is on these inputs (asserted).  The sign choice holds on the same outputs."""
    c1, c2, out, pad, la, lw, with_bias, _ = (G.I8[case] if case in G.I8 else G.I8_FORWARD[case])
    pr = G._i8_host_problem(c1, c2, out, pad, la, lw, with_bias)
    o, num = R.i8_model(pr["xidx"], pr["gq"], pr["b"], pr["a_act"], pr["a_w"], la, lw, pad)
    assert o.shape == (G.N, *out, c2) and np.abs(num).max() < 2 ** 24
    ref = _ndhwc64(pr["ref"])
    sc = float(pr["a_act"]) * float(pr["a_w"]) / ((la - 1) * (lw - 1))
    bound = 3 * U32 * (np.abs(num * sc) + (0.0 if pr["b"] is None else np.abs(pr["b"].double().numpy())))
    assert (np.abs(o.astype(np.float64) - ref) <= bound).all()
    targets, second = R.probe_targets(o)                        # the sign choice on the GPU case's own outputs
    assert 0.0 <= second < 0.5
    assert np.array_equal(np.abs(o - targets), np.full(o.shape, 0.5, np.float32))


@pytest.mark.parametrize("la,lw", [(4, 4), (128, 128), (4, 256), (256, 4), (256, 256)])
@pytest.mark.parametrize("geo", [(4, 3, 1, (0, 1, 2), (5, 6, 7)), (16, 2, 2, 1, (6, 6, 7)), (16, 1, 3, 0, (7, 8, 9))])
def test_i8s_model_reproduces_the_header_identity(la, lw, geo):
    """wmul * (acc + aoff * Ksum) + (Lw > 128 ? Su : 0) with the re-centred int8 operands and -128 in padded taps is the
    plain conv of level ids and numerators 2 * level - (Lw - 1): La <= 128 and La > 128, each with Lw <= 128 and Lw = 256."""
    c1, k, s, p, sp = geo
    gen = torch.Generator().manual_seed(la + 3 * lw + c1 + k)
    xidx = torch.randint(0, la, (2, *sp, c1), generator=gen, dtype=torch.uint8)
    m = 2 * torch.randint(0, lw, (8, c1, k, k, k), generator=gen) - (lw - 1)
    gop = R.i8s_operand(m, lw)
    assert int(gop.min()) >= -128 and int(gop.max()) <= 127
    parts = R.i8s_parts(xidx, gop, la, lw, s, p)
    assert (parts["aoff"], parts["wmul"]) == (128 if la > 128 else 0, 2 if lw > 128 else 1)
    b = torch.randn(8, generator=gen) * 0.1
    o, num = R.i8s_model(xidx, gop, b, 0.8123, 0.1, la, lw, s, p)
    want = R.int_conv(xidx, m, s, p)
    assert np.array_equal(num, want)
    if la <= 128 and lw <= 128:                                # nothing re-centred: the accumulator is the numerator
        assert np.array_equal(parts["acc"], want)
    assert np.array_equal(o, R.scale_bias(want, R.epilogue_scale(0.8123, 0.1, la, lw), b.numpy()))


def test_epilogue_scale_rounds_the_double_product_once():
    a_act, a_w = np.float32(0.8123), np.float32(0.0555)
    s = R.epilogue_scale(a_act, a_w, 16, 128)
    assert s.dtype == np.float32
    assert float(s) == float(np.float32(float(a_act) * float(a_w) * (1.0 / (15.0 * 127.0))))
    # not the float32 product, and not the division by the level product
    assert any(R.epilogue_scale(np.float32(a), a_w, 16, 128) != np.float32(np.float32(a) * a_w) / np.float32(15 * 127)
               for a in np.linspace(0.5, 1.5, 50))


@pytest.mark.parametrize("scale", [0.05, 1.0, 30.0, 300.0])
def test_probe_builder_gives_the_brute_force_float32_sums(scale):
    """Every probe of the family on random outputs: d = f32(o - y) is +-0.5 or 0 exactly, and the sums of f32(d * d) and of
    f32(att * d^2) are the builder's.  No output is outside the full set; every output is in some coordinate plane or at the
    origin."""
    gen = np.random.default_rng(int(scale * 100))
    shape = (2, 9, 7, 11, 64)
    o = (gen.standard_normal(shape) * scale).astype(np.float32)
    o[0, 0, 0, 0, :8] = [0.0, 0.25, -0.25, 0.5, -0.5, 1e-30, -1e-30, 2.0 ** -24]
    att = gen.choice(np.array([0.25, 1.0, 3.5]), size=shape[:4])
    targets, second = R.probe_targets(o)
    assert second < 0.3
    seen = np.zeros(shape, bool)
    names = []
    for name, mask in R.probe_sets(shape):
        names.append(name)
        y, s0, s1 = R.probe(o, targets, mask, att)
        d = o - y
        m = np.broadcast_to(mask, shape)
        assert np.array_equal(np.abs(d), np.where(m, np.float32(0.5), np.float32(0.0)))
        assert R.brute_force_sums(o, y, att) == (s0, s1)
        assert R.brute_force_sums(o, y, None) == (s0, s0)
        if name == "full":
            assert m.all() and s0 == 0.25 * o.size
        elif name == "zero":
            assert not m.any() and (s0, s1) == (0.0, 0.0)
        else:
            seen |= m
    assert len(names) == 2 + 1 + 4 + 3 + 4 + 6
    seen[0, 0, 0, 0, 0] = True
    assert seen.all()


def test_a_dropped_or_doubled_output_is_named_by_the_planes_that_fail():
    """The family run against a fake kernel that leaves one output out of its sum: the failing planes are those of the
    output's coordinate bits, and the message carries the coordinates."""
    gen = np.random.default_rng(5)
    shape = (2, 5, 4, 9, 32)
    o = gen.standard_normal(shape).astype(np.float32)
    hole = (1, 4, 2, 6, 19)

    def launch(y):
        d = o - y
        sq = (d * d).astype(np.float64)
        sq[hole] = 0.0
        return [sq.sum(), sq.sum()]

    with pytest.raises(AssertionError) as err:
        R.run_family(launch, o)
    msg = str(err.value)
    assert "{'n': 1, 'od': 4, 'oh': 2, 'ow': 6, 'c': 19}" in msg and "zero:" not in msg and "full:" in msg
    assert R.run_family(lambda y: list(R.brute_force_sums(o, y)), o) == 2 + 1 + 3 + 2 + 4 + 5


@pytest.mark.parametrize("case", list(G.I8S) + list(R.I8S_EXTRA))
def test_sign_choice_on_the_short_k_cases(case):
    from efficientq_amd import _lib
    from efficientq_amd import hip_ops as H
    pr = R.i8s_problem(case)
    c1, c2, k, s, p, la, lw, sp, want = R.i8s_case(case)
    G.assert_i8s_plan(H.conv_i8s_plan_query(_lib.load(), H.make_geom((G.N, c1, *sp), c2, k, s, p), la, lw), want, c1, k)
    assert np.array_equal(pr["num"], R.int_conv(pr["xidx"], pr["m"], s, p))
    R.probe_targets(pr["o"])


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_sign_choice_on_the_saturated_cases(pattern):
    """Outputs of a few hundred (512 channels, every operand at its extreme) still take one of the two signs exactly."""
    top = 0.0
    for kern, (c1, c2, _, _, with_bias, outs) in G._I8_KERNELS.items():
        pr = R.saturated_i8_problem(c1, c2, outs["p012"], G._PADS["p012"], 128, 128, with_bias, pattern)
        R.probe_targets(pr["o"])
        peak = int(np.abs(pr["num"]).max())
        assert peak == 27 * c1 * 127 * 127 if pattern in ("pos", "neg") else peak >= 27 * c1 * 127 * 127 // 4
        top = max(top, float(np.abs(pr["o"]).max()))
    assert top > (100.0 if pattern == "checker" else 200.0)
    for case in R.I8S_SATURATED:
        pr = R.i8s_problem(case, pattern)
        R.probe_targets(pr["o"])


def test_sign_choice_on_the_several_tiles_cases(monkeypatch):
    """The inputs of test_conv_tiles_gpu.I8_CASES, built by its own _i8_problem with the device replaced by the host."""
    class HostOps:
        @staticmethod
        def new_fp_state():
            return torch.zeros(5, dtype=torch.float64)

    monkeypatch.setattr(T, "DEV", "cpu")
    for case, (c1, c2, n, sp, la, lw, with_bias) in T.I8_CASES.items():
        (_, _, _, _, _, _), gq, a_w, _, _, ref, d = T._i8_problem(HostOps, case, seed=5 + sum(map(ord, case)))
        o, num = R.i8_model(d["xidx"], gq, d["b"], d["alpha"].item(), a_w, la, lw, 1)
        assert float(d["st"][0]) == float(a_w)
        R.probe_targets(o)
        assert np.abs(o.astype(np.float64) - _ndhwc64(ref)).max() <= 3 * U32 * float(ref.abs().max() + 1)
