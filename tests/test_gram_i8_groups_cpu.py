"""effq_gram_i8_group_query answers without a device, and grouping the block pairs of the i8 Gram kernel leaves the plan of
effq_gram_i8_plan_query (blocks, pairs, chunks per split, splits: what the slabs and the int32 range depend on) alone."""
import ctypes as C

import pytest

# (N, C1, D, H, W), c2, k, classes, list slots: the cases of tests/test_gram_i8_groups_gpu.py, then the benchmark's layers
GEOMS = [((2, 32, 8, 9, 10), 32, 3, 1, 0), ((2, 32, 8, 9, 10), 32, 3, 16, 20 * 128), ((1, 32, 6, 6, 6), 48, 3, 1, 0),
         ((1, 64, 4, 4, 4), 64, 3, 1, 0), ((4, 32, 16, 16, 16), 32, 3, 3, 128 * 128), ((1, 32, 8, 8, 8), 64, 1, 1, 0),
         ((1, 16, 8, 8, 8), 16, 1, 1, 0), ((1, 64, 56, 56, 65), 64, 3, 1, 0),
         ((16, 32, 64, 64, 64), 32, 3, 1, 0), ((16, 64, 32, 32, 32), 64, 3, 1, 0), ((16, 128, 16, 16, 16), 128, 3, 1, 0),
         ((16, 256, 8, 8, 8), 256, 3, 1, 0)]
# (gi, gj, ngroups, grid_y) of the rule: groups, with every split cut in two, from two block rows and 64 chunks per split
GROUPS = [(1, 1, 35, 3), (1, 1, 35, 5), (1, 1, 42, 1), (1, 1, 133, 1), (1, 1, 35, 32), (1, 1, 3, 1), (1, 1, 1, 1),
          (2, 2, 35, 48),
          (2, 2, 10, 176), (2, 2, 35, 48), (2, 2, 133, 12), (1, 1, 1980, 2)]


@pytest.fixture()
def lib():
    from efficientq_amd import _lib
    lib = _lib.load()
    yield lib
    lib.effq_gram_i8_set_group(0, 0)


def _queries(lib, shape, c2, k, ncls, n_list):
    from efficientq_amd.hip_ops import make_geom
    g = make_geom(shape, c2, k, 1, k // 2)
    plan, grp = [C.c_int() for _ in range(6)], [C.c_int() for _ in range(4)]
    assert lib.effq_gram_i8_plan_query(C.byref(g), ncls, n_list, *[C.byref(o) for o in plan]) == 0
    assert lib.effq_gram_i8_group_query(C.byref(g), ncls, n_list, *[C.byref(o) for o in grp]) == 0
    return tuple(o.value for o in plan), tuple(o.value for o in grp)


def _plan_formulas(shape, c2, k, n_list):
    """NB, NBX, npairs, nchunks, cps, nsplit as the parent commit plans them (gram_i8_plan)."""
    N, c1, D, H, W = shape
    rx = k ** 3 * c1
    yr0 = rx + 16
    E = yr0 + 4 * ((c2 + 15) // 16 * 16)
    NB, NBX = (E + 127) // 128, (yr0 + 127) // 128
    npairs = NBX * NB - NBX * (NBX - 1) // 2
    nchunks = n_list // 128 if n_list else (N * D * H * W + 127) // 128
    want = max(1, min((3072 + npairs - 1) // npairs, nchunks // 4))
    cps = min((nchunks + want - 1) // want, 1000)
    return NB, NBX, npairs, nchunks, cps, (nchunks + cps - 1) // cps


@pytest.mark.parametrize("geom,groups", list(zip(GEOMS, GROUPS)), ids=[f"{g[0][1]}to{g[1]}-k{g[2]}-{i}" for i, g in enumerate(GEOMS)])
def test_group_query_and_unchanged_plan(lib, geom, groups):
    shape, c2, k, ncls, n_list = geom
    want_plan = _plan_formulas(shape, c2, k, n_list)
    plan, grp = _queries(lib, *geom)
    assert plan == want_plan
    assert grp == groups
    NB, NBX, npairs, _, cps, nsplit = plan
    G = 2 if NBX >= 2 and cps >= 64 else 1                         # the rule
    assert grp == (G, G, sum((NB - i0 + G - 1) // G for i0 in range(0, NBX, G)), nsplit * G)
    # the override changes the groups and nothing of the plan
    assert lib.effq_gram_i8_set_group(1, 1) == 0
    plan1, grp1 = _queries(lib, *geom)
    assert plan1 == want_plan and grp1 == (1, 1, npairs, nsplit)
    assert lib.effq_gram_i8_set_group(2, 2) == 0
    plan2, grp2 = _queries(lib, *geom)
    assert plan2 == want_plan and grp2 == (2, 2, sum((NB - i0 + 1) // 2 for i0 in range(0, NBX, 2)),
                                           nsplit * (2 if cps >= 64 else 1))
    assert lib.effq_gram_i8_set_group(0, 0) == 0
    assert _queries(lib, *geom) == (plan, grp)


def test_group_override_rejects_other_shapes(lib):
    for bad in [(2, 1), (1, 2), (3, 3), (-1, -1), (0, 1)]:
        assert lib.effq_gram_i8_set_group(*bad) == 1               # EFFQ_ERR_ARG
    v = C.c_int()
    from efficientq_amd.hip_ops import make_geom
    g = make_geom((1, 16, 8, 8, 8), 16, 1, 1, 0)
    assert lib.effq_gram_i8_group_query(C.byref(g), 1, 130, C.byref(v), C.byref(v), C.byref(v), C.byref(v)) == 1
    assert lib.effq_gram_i8_group_query(C.byref(g), 1, 0, None, C.byref(v), C.byref(v), C.byref(v)) == 1
