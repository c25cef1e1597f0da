"""--gptq_refine / --gptq_order, host side (no GPU): the numpy statement of the passes against the direct quadratic form and
a brute-force search, the ordering, the refusals, and the seeds of tests/test_gptq_refine_gpu.py."""
import argparse

import numpy as np
import pytest

from efficientq_amd import config as Cf, entrance, gptq
from tests.gptq_refine_ref import CASES, EXCUSED, quad, system, threshold


def _sweep_state(H, u, alpha, levels, bias):
    q, ids, err = gptq.sweep_host(gptq.factor_host(H), u, alpha, levels, bias)
    return ids[:, :u.shape[1] - int(bias)], (q[:, -1] if bias else None), err


@pytest.mark.parametrize("block", [4, 64])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("levels", [2, 4])
def test_every_pass_lowers_the_quadratic_form_and_ends_coordinate_wise_optimal(levels, bias, block):
    n = 11 + int(bias)
    _, H, u, alpha = system(n, bias, 8, False)
    ids, b, err = _sweep_state(H, u, alpha, levels, bias)
    for _ in range(20):
        q, ids, moves, errs, _ = gptq.refine_host(H, u, ids, b, alpha, levels, bias, 1, block=block)
        b = q[:, -1] if bias else None
        assert np.all(np.abs(errs[0] - quad(H, q, u)) <= 1e-12 * errs[0]) and np.all(errs[0] <= err * (1 + 1e-12))
        err = errs[0]
        if moves.sum() == 0:
            break
    assert moves.sum() == 0
    for j in range(n - int(bias)):          # no other grid value of any one weight is better
        for v in alpha[0] * (np.arange(levels) * 2.0 / (levels - 1) - 1.0):
            alt = q.copy()
            alt[:, j] = v
            assert np.all(quad(H, alt, u) >= err * (1 - 1e-12))


def test_order_host_sorts_descending_keeps_ties_in_order_and_the_bias_last():
    d = np.array([3.0, 5.0, 3.0, 9.0, 5.0, 1.0])
    assert gptq.order_host(d, False).tolist() == [3, 1, 4, 0, 2, 5]
    assert gptq.order_host(d, True).tolist() == [3, 1, 4, 0, 2, 5]         # the last entry is the bias: it stays
    assert gptq.order_host(np.array([1.0, 2.0, 99.0]), True).tolist() == [1, 0, 2]


@pytest.mark.parametrize("over,match", [
    (dict(qconv="effq", gptq_refine=2), r"--gptq_refine 2.*--qconv is effq"),
    (dict(qconv="conv", gptq_order="act"), r"--gptq_order act.*--qconv is conv"),
    (dict(qconv="gptq", gptq_refine=17), r"--gptq_refine 17.*0 to 16"),
    (dict(qconv="gptq", gptq_refine=-1), r"--gptq_refine -1"),
    (dict(qconv="gptq", gptq_order="random"), r"--gptq_order 'random'.*natural, act")])
def test_switches_are_refused_by_name(over, match):
    with pytest.raises(SystemExit, match=match):
        Cf.get_conv_class(Cf.make_args(dict(Cf.TINY_NET, **over), 4, 4))
    with pytest.raises(SystemExit, match=match):
        entrance.main(["ptq"] + [f"--{k}={v}" for k, v in over.items()])
    assert Cf.gptq_switches(argparse.Namespace(qconv="effq")) == {}
    kwQ = Cf.get_conv_class(Cf.make_args(dict(Cf.TINY_NET, qconv="gptq", gptq_refine=3, gptq_order="act"), 4, 4))[2]
    assert (kwQ["gptq_refine"], kwQ["gptq_order"]) == (3, "act")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n=%d,bias=%d,c2=%d,L=%d,rows=%d,K=%d" % c)
def test_the_host_walk_of_every_gpu_case_moves_columns_and_stays_clear_of_its_margin(case):
    n, bias, c2, levels, per_row, passes = case
    _, H, u, alpha = system(n, bias, c2, per_row)
    ids, b, err = _sweep_state(H, u, alpha, levels, bias)
    q, _, moves, errs, margin = gptq.refine_host(H, u, ids, b, alpha, levels, bias, passes)
    excused = margin < threshold(H, q, u, alpha, passes)
    print(f"{case}: moves {int(moves.sum())}, err {err.sum():.6g} -> {errs[-1].sum():.6g}, excused {int(excused.sum())}")
    assert moves.sum() >= 1 and excused.sum() <= EXCUSED * c2 and np.all(errs[-1] <= err * (1 + 1e-12))
