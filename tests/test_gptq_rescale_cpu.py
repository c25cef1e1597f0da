"""--gptq_rescale, host side (no GPU): gptq.rescale_host against a least-squares fit of (alpha, beta) in the H norm with the
ids fixed, its guards, the descent of [refit, pass] rounds, and the refusals."""
import numpy as np
import pytest

from efficientq_amd import config as Cf, entrance, gptq
from tests.gptq_refine_ref import quad, system


def _state(n, bias, c2, per_row, levels=4):
    _, H, u, alpha = system(n, bias, c2, per_row)
    q, ids, err = gptq.sweep_host(gptq.factor_host(H), u, alpha, levels, bias)
    return H, u, alpha, ids[:, :n - int(bias)], (q[:, -1] if bias else None), err


def _lstsq(H, u, ids, levels, bias, per_row):
    """(alpha (c2), beta (c2, n_bias), err (c2)): min over alpha (one per row, or one for all) and every row's beta of
    sum_r ||R ([alpha v_r | beta_r] - u_r)||^2 with H = R^T R."""
    c2, n = u.shape
    R = np.linalg.cholesky(H).T
    v = np.zeros((c2, n))
    v[:, :ids.shape[1]] = ids * (2.0 / (levels - 1)) - 1.0
    na = c2 if per_row else 1
    M = np.zeros((c2 * n, na + c2 * int(bias)))
    for r in range(c2):
        M[r * n:(r + 1) * n, r if per_row else 0] = R @ v[r]
        if bias:
            M[r * n:(r + 1) * n, na + r] = R[:, -1]
    x = np.linalg.lstsq(M, (u @ R.T).reshape(-1), rcond=None)[0]
    alpha, beta = np.broadcast_to(x[:na], (c2,)), x[na:].reshape(c2, int(bias))
    return alpha, beta, quad(H, np.concatenate([alpha[:, None] * v[:, :ids.shape[1]], beta], axis=1), u)


@pytest.mark.parametrize("per_row", [True, False], ids=["rows", "tensor"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_refit_is_the_least_squares_scale_in_the_h_norm(bias, per_row):
    H, u, alpha, ids, b, err0 = _state(13, bias, 6, per_row)
    a, bn, err, kept = gptq.rescale_host(H, u, ids, b, alpha, 4, bias, per_row)
    want_a, want_b, want_err = _lstsq(H, u, ids, 4, bias, per_row)
    assert kept == 0 and a.shape == ((6,) if per_row else (1,))
    assert np.all(np.abs(a - want_a[:a.size]) <= 1e-10 * want_a[:a.size]) and np.all(np.abs(err - want_err) <= 1e-9 * want_err)
    assert (bn is None) if not bias else np.all(np.abs(bn - want_b[:, 0]) <= 1e-10 * np.abs(want_b[:, 0]).max())
    assert np.all(err <= err0 * (1 + 1e-12)) if per_row else err.sum() <= err0.sum() * (1 + 1e-12)
    assert err.sum() < err0.sum()


def test_a_refit_that_is_no_positive_scale_is_not_taken():
    H, u, alpha, ids, b, _ = _state(13, True, 6, True)
    u, ids, flag = u.copy(), ids.copy(), np.zeros(6, dtype=np.int32)
    u[1], ids[1] = 0.0, 2                                    # c1 = 0 although v H v^T > 0
    u[2, :-1] = -(ids[2] * (2.0 / 3) - 1.0)                  # c1 < 0
    flag[4] = 1
    a, bn, err, kept = gptq.rescale_host(H, u, ids, b, alpha, 4, True, True, row_flag=flag)
    bad, good = [1, 2, 4], [0, 3, 5]
    assert kept == 3 and np.array_equal(a[bad], alpha[bad]) and np.array_equal(bn[bad], b[bad])
    assert np.all(a[good] != alpha[good]) and np.all(a[good] > 0)
    q = np.concatenate([a[:, None] * (ids * (2.0 / 3) - 1.0), bn[:, None]], axis=1)
    assert np.all(np.abs(err - quad(H, q, u)) <= 1e-9 * err)           # err is f at the point every row stands on
    # per tensor one flagged row keeps the whole tensor
    a, bn, _, kept = gptq.rescale_host(H, u, ids, b, alpha[:1], 4, True, False, row_flag=flag)
    assert kept == 1 and a[0] == alpha[0] and np.array_equal(bn, b)


@pytest.mark.parametrize("per_row", [True, False], ids=["rows", "tensor"])
def test_rounds_of_refit_and_pass_never_raise_the_error(per_row):
    H, u, alpha, ids, b, err = _state(29, True, 6, per_row)
    moved = 0
    for _ in range(3):
        alpha, b, e1, kept = gptq.rescale_host(H, u, ids, b, alpha, 4, True, per_row)
        q, ids, moves, errs, _ = gptq.refine_host(H, u, ids, b, alpha, 4, True, 1)
        for new in (e1, errs[-1]):
            assert kept == 0 and (np.all(new <= err * (1 + 1e-12)) if per_row else new.sum() <= err.sum() * (1 + 1e-12))
            err = new
        b, moved = q[:, -1], moved + int(moves.sum())
    assert moved >= 1


@pytest.mark.parametrize("over,match", [
    (dict(qconv="effq", gptq_rescale=1), r"--gptq_rescale 1.*--qconv is effq"),
    (dict(qconv="gptq", gptq_rescale=9), r"--gptq_rescale 9.*0 to 8"),
    (dict(qconv="gptq", gptq_rescale=-1), r"--gptq_rescale -1"),
    (dict(qconv="gptq", gptq_rescale=2), r"--gptq_rescale 2 with gptq_refine 0")])
def test_the_switch_is_refused_by_name(over, match):
    with pytest.raises(SystemExit, match=match):
        Cf.get_conv_class(Cf.make_args(dict(Cf.TINY_NET, **over), 4, 4))
    with pytest.raises(SystemExit, match=match):
        entrance.main(["ptq"] + [f"--{k}={v}" for k, v in over.items()])
    with pytest.raises(ValueError, match="gptq_rescale"):
        gptq.check_options(0, "natural", over["gptq_rescale"] if over["qconv"] == "gptq" else 1.5)
    assert gptq.check_options(2, "act", 2) == (2, "act", 2) and gptq.check_options(0, "natural") == (0, "natural", 0)
    kwQ = Cf.get_conv_class(Cf.make_args(dict(Cf.TINY_NET, qconv="gptq", gptq_refine=1, gptq_rescale=3), 4, 4))[2]
    assert (kwQ["gptq_refine"], kwQ["gptq_rescale"]) == (1, 3)
