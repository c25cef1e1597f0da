"""tests/fp_traj_ref.py, the fp64 restatement of effq_fixed_point_traj that tests/test_fp_traj_classes_gpu.py holds the
kernel to, checked without a GPU: its loop is oracle.effq_oracle.fit_scale's to the last bit, and its seven-call
schedules reach every way the kernel serves an iterate, none of them by a margin a rounding could flip."""
import math

import numpy as np
import pytest
import torch

from tests import fp_traj_ref as R
from oracle import effq_oracle as O

TOL = 1e-5


def _tensors(L):
    out = {"random": R.normal(20001, 11 + L), "clustered": R.clustered(16385, 12 + L), "one": R.normal(1, 13),
           "odd": R.normal(4097, 14 + L, sigma=3.0)}
    out.update(R.adversarial(L))
    return out


@pytest.mark.parametrize("L", [2, 3, 4, 16])
def test_iterates_is_the_oracles_loop_to_the_last_bit(L):
    checked = 0
    for name, v in _tensors(L).items():
        got = R.iterates(v, L, -1.0, 1.0, TOL, 100 * L)
        try:
            fit = O.fit_scale(torch.from_numpy(v), L, -1, 1)
        except RuntimeWarning:
            assert got["done"] == 2 and got["it"] == 100 * L, name
            continue
        assert got["done"] == 1 and got["it"] == fit.iters, (name, got["it"], fit.iters)
        assert got["alpha"] == fit.alpha, (name, got["alpha"], fit.alpha)
        assert len(got["alphas"]) == got["it"] and got["alphas"][0] == float(torch.from_numpy(v).double().abs().mean())
        checked += 1
    assert checked >= 8


def test_cap_semantics_are_fp_stops():
    v = R.clustered(16385, 5)
    full = R.iterates(v, 4, -1.0, 1.0, TOL, 400)
    assert full["done"] == 1 and full["it"] >= 4
    cut = R.iterates(v, 4, -1.0, 1.0, TOL, 3)
    assert (cut["done"], cut["it"]) == (2, 3) and cut["alphas"] == full["alphas"][:3] and cut["alpha"] == full["alphas"][3]
    # the cap wins even where the last step converged
    at = R.iterates(v, 4, -1.0, 1.0, TOL, full["it"])
    assert (at["done"], at["it"], at["alpha"]) == (2, full["it"], full["alpha"])
    zero = R.iterates(np.zeros(100, np.float32), 4, -1.0, 1.0, TOL, 400)
    assert (zero["done"], zero["it"], zero["alphas"]) == (2, 0, [])


def test_record_follows_the_recorders_rules():
    p0 = R.cold_pred()
    p1 = R.record(p0, [0.1, 0.2, 0.3], 0.31, 1000.0, 4)
    assert p1["K"] == 3 and p1["lo"][:3] == [0.1, 0.2, 0.3] and p1["hi"][:3] == [0.1, 0.2, 0.31]
    assert p1["eps"][:3] == [0.01] * 3 and p1["eps_n"][:3] == [0.01] * 3 and p1["eps"][3] == 0.0
    assert p1["e_valid"] == 1 and p1["e"] == 58 - 11                              # 3000 = 1.46 * 2^11
    p2 = R.record(p1, [0.1, 0.21], 0.21, 1000.0, 4)                                 # drifts 0 and 0.01 / 0.21: past the cap
    assert p2["K"] == 2 and p2["eps"][0] == 0.0085 and p2["eps_n"][0] == 1e-4
    assert p2["eps"][1] == 0.03 and p2["eps_n"][1] == 0.03 and p2["lo"][2] == 0.3   # slot 2 keeps what it held
    ten = [0.1 + 0.01 * i for i in range(10)]
    p3 = R.record(p0, ten, 0.05, 0.0, 4)
    assert p3["K"] == 8 and p3["lo"][7] == 0.05 and p3["hi"][7] == ten[9] and (p3["e"], p3["e_valid"]) == (0, 0)
    p4 = R.record(dict(p1, K=9), [0.1], 0.1, 1000.0, 4)                            # an impossible K is not trusted
    assert p4["eps"][0] == 0.01


def _walk(n, L, kind):
    base, pred, calls = R.schedule_base(n, L, kind), R.cold_pred(), []
    for k in range(len(R.SCHEDULE)):
        v = R.scheduled(base, k)
        fit = R.iterates(v, L, -1.0, 1.0, TOL, 100 * L)
        cls = R.classify(pred, v, L, -1.0, 1.0, fit["alphas"])
        calls.append((fit, cls))
        pred = R.record(pred, fit["alphas"], fit["alpha"], fit["sum_abs"], L)
    return calls


@pytest.fixture(scope="module")
def walks():
    return {case: _walk(*case) for case in R.SCHEDULE_CASES}


@pytest.mark.parametrize("case", R.SCHEDULE_CASES, ids=lambda c: f"{c[0]}-L{c[1]}")
def test_schedule_reaches_its_classes_with_margins(walks, case):
    calls = walks[case]
    n, L, _ = case
    print()
    for k, (fit, cls) in enumerate(calls):
        print(f"n={n} L={L} call {k}: it={fit['it']} m_n={cls['m_n']} m_r={cls['m_r']} classes={cls['classes']} "
              f"bracket_margin={cls['bracket_margin']:.2e} stop_margin={fit['stop_margin']:.2e}")
        assert fit["done"] == 1 and fit["stop_margin"] > 1e-9
        assert cls["bracket_margin"] > 1e-9
        assert cls["m_n"] + cls["m_r"] <= n
    kinds = [set(cls["classes"]) for _, cls in calls]
    assert kinds[0] == {"f"} and not calls[0][1]["warm"]                           # cold
    assert kinds[1] == {"n"} and kinds[2] == {"n"} and kinds[5] == {"n"} and kinds[6] == {"n"}
    assert "r" in kinds[3] and "f" in kinds[4] and calls[4][1]["tallies_ok"]
    if L <= 4:
        assert kinds[3] == {"r"} and kinds[4] == {"f"}
    else:
        assert len(kinds[3]) >= 2 and len(kinds[4]) >= 2                          # several ways inside one call


def test_schedules_cover_every_class_between_them(walks):
    got = set()
    for calls in walks.values():
        for fit, cls in calls:
            got |= R.reached(cls, fit["it"])
    assert got == set(R.REQUIRED), set(R.REQUIRED) - got


def test_classify_lists_a_value_on_a_boundary_and_settles_one_far_from_it():
    L, d = 4, 2.0 / 3.0
    pred = R.record(R.cold_pred(), [0.07], 0.07, 1000.2, L)                         # one slot at 0.07, margins 1 %
    on, off = np.float32(0.07 * (0.5 * d - 1.0)), np.float32(0.07 * (1.0 * d - 1.0))   # a boundary, a level centre
    v = np.array([on, off, 0.0, 500.0, -500.0], np.float32)                        # zero sits on the boundary 1 | 2 at EVERY scale: settled
    cls = R.classify(pred, v, L, -1.0, 1.0, [0.07, 0.0705, 0.08])
    assert (cls["m_n"], cls["m_r"], cls["classes"]) == (1, 0, "nnf") and cls["tallies_ok"]
    assert math.isclose(cls["bracket_margin"], (0.07 * 1.01 - 0.0705) / 0.0705, rel_tol=1e-9)
    # ring: narrower narrow margin, a value between the two brackets' reach
    pred["eps_n"][0] = 1e-4
    mid = np.float32(0.07 * 1.005 * (0.5 * d - 1.0))
    cls = R.classify(pred, np.array([on, mid, off, 500.0, -500.0], np.float32), L, -1.0, 1.0, [0.07 * 1.002])
    assert (cls["m_n"], cls["m_r"], cls["classes"]) == (1, 1, "r")


def test_classify_trusts_no_field_that_is_not_a_record():
    """A slot whose ends are not positive and ordered is dead (the level is monotone in the scale on a > 0 only; phase 2
    takes narrow inside wide for granted), and so are the tallies of a unit that is not this tensor's to within 4 x."""
    L, v = 4, R.clustered(4097, 9)
    fit = R.iterates(v, L, -1.0, 1.0, TOL, 400)
    good = R.record(R.cold_pred(), fit["alphas"], fit["alpha"], fit["sum_abs"], L)
    assert set(R.classify(good, v, L, -1.0, 1.0, fit["alphas"])["classes"]) == {"n"}
    for field, value in (("eps", [-0.5] * 8), ("lo", [-x for x in good["lo"]]), ("hi", [0.0] * 8), ("hi", [math.inf] * 8)):
        cls = R.classify(dict(good, **{field: value}), v, L, -1.0, 1.0, fit["alphas"])
        assert (cls["m_n"], cls["m_r"], set(cls["classes"])) == (0, 0, {"f"}), field
    for e in (good["e"] - 3, good["e"] + 3, -2000000000, 2000000000):
        cls = R.classify(dict(good, e=e), v, L, -1.0, 1.0, fit["alphas"])
        assert not cls["tallies_ok"] and set(cls["classes"]) == {"f"}
    assert R.classify(dict(good, e=good["e"] - 2), v, L, -1.0, 1.0, fit["alphas"])["tallies_ok"]
