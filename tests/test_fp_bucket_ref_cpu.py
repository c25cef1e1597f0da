"""tests/fp_bucket_ref.py, the numpy restatement of effq_fixed_point_bucket's dispatch that
tests/test_fp_bucket_classes_gpu.py runs its cases by, checked without a GPU: the loop is the oracle's, the kernel's counting
rule (v <= the band's lower end, the reference's arithmetic inside the band) gives the direct count level_exact < k for
every case on both grids, every row of the table reaches the classes it is there for, every class has a row, and no row's
iteration count hangs on a rounding."""
import functools

import numpy as np
import pytest
import torch

from tests import fp_bucket_ref as F
from tests import fp_traj_ref as R
from oracle import effq_oracle as O

GRIDS = ((-1.0, 1.0), (0.0, 1.0))


@functools.lru_cache(maxsize=None)
def _fit(case, lo, hi):
    return R.iterates(F.tensor(case.spec), case.levels, lo, hi, F.TOL, 100 * case.levels)


@functools.lru_cache(maxsize=None)
def _classes(case):
    return F.classes(F.tensor(case.spec), case.levels, case.lo, case.hi, fit=_fit(case, case.lo, case.hi))


def _by_name(name):
    return next(c for c in F.CASES if c.name == name)


@pytest.mark.parametrize("name", ["normal-8193", "L16-12000", "relu-L4-12000"])
def test_iterates_is_the_oracles_loop(name):
    case = _by_name(name)
    got = _fit(case, case.lo, case.hi)
    fit = O.fit_scale(torch.from_numpy(F.tensor(case.spec)), case.levels, case.lo, case.hi)
    assert (got["done"], got["it"]) == (1, fit.iters)
    assert np.float64(got["alpha"]).view(np.int64) == np.float64(fit.alpha).view(np.int64)


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.name)
def test_the_counting_rule_is_the_direct_count(case):
    """The design claim of the kernel's header, on every case and both grids: counting whole buckets and values outside
    the guard band by comparison, and the values inside it by the reference's arithmetic, is counting level_exact < k."""
    v = F.tensor(case.spec)
    for lo, hi in GRIDS:
        try:
            fit = _fit(case, lo, hi)
        except ZeroDivisionError:
            # no value above the first boundary of the unsigned grid (one negative value): sum b^2 = 0, no fixed point
            assert (lo, hi) != (case.lo, case.hi) and not (v > 0).any()
            continue
        rule = F.counts_by_rule(v, case.levels, lo, hi, fit=fit)
        direct = F.counts_direct(v, case.levels, lo, hi, fit=fit)
        assert rule.shape == direct.shape == (fit["it"], case.levels - 1)
        assert np.array_equal(rule, direct), (case.name, lo, np.argwhere(rule != direct)[:5])


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.name)
def test_a_case_reaches_the_classes_it_is_there_for(case):
    cls = _classes(case)
    got = F.reached(cls)
    print(f"\n{case.name}: n={cls['geometry'].n} it={cls['fit']['it']} {sorted(got)} "
          f"{ {k: x for k, x in cls['tallies'].items() if x} }")
    assert set(case.reaches) <= got, set(case.reaches) - got
    assert sum(cls["tallies"][k] for k in F.TALLIES[:3]) == cls["pairs"]      # every pair has exactly one segment class


def test_every_class_has_a_case_that_is_there_for_it():
    named = set()
    for case in F.CASES:
        named |= set(case.reaches)
    assert named >= set(F.REQUIRED), set(F.REQUIRED) - named


def test_the_table_holds_the_cases_of_the_sections():
    names = [c.name for c in F.CASES]
    assert len(set(names)) == len(names)
    a = F.section("a")
    assert sorted({F.tensor(c.spec).size for c in a if c.spec[1] < F.MAXN}) == sorted(F.A_SIZES)
    assert [c.spec[1] for c in a].count(F.MAXN) == 1                            # the admitted maximum, once
    assert {c.levels for c in F.section("b")} == set(F.B_LEVELS)
    assert {F.geometry(F.tensor(c.spec)).path for c in F.section("b") if c.levels == 9} == {"S", "G"}
    assert {(c.lo, c.hi) for c in F.section("d")} == {(0.0, 1.0)}
    for case in F.section("d"):
        v = F.tensor(case.spec)
        if case.spec[0] == "relu":
            assert np.count_nonzero(v == 0) >= v.size // 3 and np.signbit(v).any() and (np.abs(v[v != 0]) < 1e-38).any()
        else:
            assert np.count_nonzero(v < 0) >= v.size // 3


def test_the_outlier_ladder_walks_the_finer_units():
    for r, extra in F.LADDER:
        g = F.geometry(F.tensor(_by_name(f"outlier-x{r}").spec))
        assert (g.path, g.inst, g.extra) == ("S", 16, extra), (r, g.ratio)
        # (the kernel adds sum|v| in another order: the ratio must not sit on a power of two)
        assert abs(np.log2(g.ratio) - round(np.log2(g.ratio))) > 1e-3, g.ratio


def test_no_iteration_count_hangs_on_a_rounding():
    """The rule of test_fp_traj_classes_gpu._hold: a case is compared on its iteration count only where every stop
    decision is further than 1e-9 from the tolerance.  The table is built so that none fails it."""
    weak = [c.name for c in F.CASES if not _fit(c, c.lo, c.hi)["stop_margin"] > 1e-9]
    assert not weak, weak
    assert all(_fit(c, c.lo, c.hi)["done"] == 1 for c in F.CASES)


def test_the_recorded_unit_does_not_hang_on_a_rounding():
    """The recorder's e = 58 - ilogb((L - 1) sum|v|) is compared exactly, and the kernel adds sum|v| in another order."""
    for c in F.CASES:
        m = np.frexp((c.levels - 1) * _fit(c, c.lo, c.hi)["sum_abs"])[0]
        assert 0.5 + 1e-9 < m < 1.0 - 1e-9, (c.name, m)


def test_the_geometry_of_the_paths():
    assert [(F.geometry(np.ones(n, np.float32)).path, F.geometry(np.ones(n, np.float32)).inst)
            for n in (1, 8192, 8193, 16384, 16385, 32768, 32769)] == \
        [("S", 8), ("S", 8), ("S", 16), ("S", 16), ("S", 32), ("S", 32), ("G", None)]
    g = F.geometry(np.ones(32769, np.float32))
    assert (g.sum_blocks, g.count_slices, 32769 - 4 * F.SLICE) == (17, 5, 1)
    assert F.geometry(np.ones(40960, np.float32)).count_slices * F.SLICE == 40960
    assert F.geometry(np.ones(4, np.float32)).sum_blocks == 0 and -(-F.MAXN // F.SUM_WG) == F.MAXBLK
    assert [F.gs_of(L) for L in (2, 5, 6, 9, 10, 17, 18, 33, 34, 65, 66, 129, 130, 256)] == \
        [64, 64, 32, 32, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1]
    # the bucket function: monotone, the ends clamped, zero in the middle
    g = F.geometry(np.array([-0.5, 0.25], np.float32))
    assert (g.B, float(g.R)) == (2048, 0.5) and g.bucket(np.float32(-0.5)) == 0 and g.bucket(np.float32(0.5)) == 2047
    assert g.bucket(np.float32(0.0)) == 1024 and g.bucket(np.float32(-1e-30)) == 1024 and g.bucket(np.float32(-7.0)) == 0
    assert F.fpb_step(np.float32(0.0), -1).view(np.uint32) == 0x80000000      # +0 steps down to -0
    assert F.fpb_step(np.float32(1.0), +1) == np.nextafter(np.float32(1.0), np.float32(2.0))
    assert F.fpb_step(np.float32(-3.4028235e38), -1) == np.float32(-3.4028235e38)


def test_the_workspace_layout_adds_up():
    for n in (32769, 1 << 23):
        lay = F.workspace_layout(n)
        # fpg_ws_bytes, written out: header, cnt, isum, off, spre, partials, the segment tables, rank + grouped
        want = (256 + 4 * 65536 + 8 * 65536 + 4 * (65536 + 2) + 8 * (65536 + 2) + 8 * 2 * 4096 + 4096 + (4 + 4) * (n + 64))
        assert lay.total == want
        assert lay.header == (0, 256) and lay.tickets == (4, 16) and lay.isum == (256, 256 + 8 * 65536)
        assert lay.cnt[1] - lay.cnt[0] == 4 * 65536 and lay.tail == (want - 8 * (n + 64), want)
        assert lay.isum[1] <= lay.cnt[0] and lay.cnt[1] <= lay.tail[0]
    assert F.workspace_layout(32768).total == 256
