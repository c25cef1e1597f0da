"""--qconv gptq, host side (no GPU): the registry and the blocked host statement of the rule against the plain one."""
import numpy as np
import pytest

from efficientq_amd import config as Cf, gptq
from tests.gptq_ref import gptq_ref


def test_gptq_resolves_in_the_registry_and_an_unknown_name_is_refused():
    args = Cf.make_args(dict(Cf.TINY_NET, qconv="gptq"), 4, 4)
    cls, info, _ = Cf.get_conv_class(args)
    assert cls is gptq.GPTQConvHIP is Cf.QCONV_REGISTRY["gptq"] and info.startswith("gptq_")
    assert issubclass(cls, Cf.QCONV_REGISTRY["effq"]) and "QConv" in cls.__name__
    args.qconv = "obq"
    with pytest.raises(RuntimeError, match="Unknown QConv name"):
        Cf.get_conv_class(args)


@pytest.mark.parametrize("has_bias,alpha,block", [(True, 0.4, 64), (False, 0.4, 8), (True, [0.3, 0.35, 0.4], 8)])
def test_blocked_host_rule_agrees_with_the_plain_one(has_bias, alpha, block):
    rng = np.random.default_rng(3)
    n = 27 + int(has_bias)
    X = rng.integers(-3, 4, (4 * n, n)).astype(np.float64)
    if has_bias:
        X[:, -1] = 1.0
    H = 2.0 * X.T @ X + 8.0 * np.eye(n)
    u = rng.integers(-511, 512, (3, n)) / 1024.0
    P, q, ids, err, margin = gptq_ref(H, u, alpha, 4, has_bias)
    assert margin.min() > 1e-8
    assert np.abs(gptq.factor_host(H) - P).max() == 0.0
    q2, ids2, err2 = gptq.sweep_host(P, u, alpha, 4, has_bias, block=block)
    assert np.array_equal(ids2, ids)
    assert np.abs(q2 - q).max() <= 1e-12 and np.abs(err2 - err).max() <= 1e-9 * err.max()
    # err is the quadratic form of the rounding error
    assert np.abs(np.einsum("ri,ij,rj->r", q - u, H, q - u) - err).max() <= 1e-9 * err.max()
