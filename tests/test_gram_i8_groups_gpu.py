"""The block groups of the i8 Gram kernel (csrc/gram_i8.hip, k_gram_i8<2>) against fp64 and against one pair per workgroup
(-m gpu).

A workgroup of effq_gram_accum_i8 may compute a 2 x 2 group of adjacent 128-row blocks from rows it stages once, and a
planned split may be cut into two workgroups; which workgroup computes a pair must not show in any output bit (the sums
are exact integers).  The dispatch rule asks for two block rows and 64 chunks per split, which only the last case here
has, so every other case with two block rows forces the groups through effq_gram_i8_set_group(2, 2).  Every case asserts
the rule's pick through effq_gram_i8_group_query and then, under the groups (and under the rule's pick where that differs):
  Au equal to the fp64 integer reference, A0 / B0 / Bu within the 2e-7 / 2e-7 / 2e-8 bars of tests/test_gram_shapes_gpu.py
  (its _check_i8, which also asserts A0 == A0.T and that a second run on a workspace filled with 0xFF gives the same bits),
  and A0, B0, Au, Bu bit-identical between the rule's pick, the groups and effq_gram_i8_set_group(1, 1), the launch of
  one pair per workgroup.
The shapes are the smallest with the edge in question: a last I group of one block with the ones cell and the y digits
starting mid-block (NB 8, NBX 7), an odd block count (NB 9), fewer chunks than pipeline stages (one chunk, 133 pairs), K
splits with the last chunk of a class inside a split, systems with one block row, which keep one pair per workgroup, and
splits of 67 chunks cut into parts of 33 and 34."""
import pytest
import torch

from tests.test_gram_shapes_gpu import DEV, _check_i8, _geom, _same_bits, dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_ops(DEV)


def _ngroups(NB, NBX, G):
    return sum((NB - I0 + G - 1) // G for I0 in range(0, NBX, G))


def _case(ops, tag, shape, c2, k, idx, y, att, cls, want_plan, want_group, want_sub=1, La=4, alpha=0.7312):
    """One geometry: the plan and the rule's pick asserted, the checks of the module docstring."""
    geom = _geom(shape, c2, k, 1, k // 2)
    n_list = 0 if cls[0] is None else cls[0].numel()
    al = torch.tensor(alpha, dtype=torch.float32, device=DEV)
    run = lambda: ops.gram_i8(dev(idx), cls, dev(y), geom, True, al, La, unweighted=True)
    ops.gram_i8_set_group(0, 0)
    plan = ops.gram_i8_plan(geom, cls[3], n_list)
    for key, v in want_plan.items():
        assert plan[key] == v, (key, plan)
    G = want_group
    grp = ops.gram_i8_groups(geom, cls[3], n_list)
    assert grp == dict(gi=G, gj=G, ngroups=_ngroups(plan["NB"], plan["NBX"], G), grid_y=want_sub * plan["nsplit"]), grp
    settings = [(0, 0)] + ([(2, 2)] if plan["NBX"] >= 2 and G != 2 else [])
    outs = []
    try:
        for setting in settings:
            ops.gram_i8_set_group(*setting)
            now = ops.gram_i8_groups(geom, cls[3], n_list)
            if setting == (2, 2):
                assert now == dict(gi=2, gj=2, ngroups=_ngroups(plan["NB"], plan["NBX"], 2), grid_y=plan["nsplit"]), now
            _check_i8(ops, f"groups {tag} {now}", idx, y, att, cls, geom, k, 1, k // 2, True, alpha, La, cross_check=False)
            outs.append(run())
        ops.gram_i8_set_group(1, 1)
        one = ops.gram_i8_groups(geom, cls[3], n_list)
        assert one == dict(gi=1, gj=1, ngroups=plan["npairs"], grid_y=plan["nsplit"]), one
        assert ops.gram_i8_plan(geom, cls[3], n_list) == plan
        ref = run()
    finally:
        ops.gram_i8_set_group(0, 0)
    for got in outs:
        for name, a, b in zip(("A0", "B0", "Au", "Bu"), got, ref):
            assert _same_bits(a, b), f"{name} differs between the groups and one pair per workgroup"


def _data(shape, c2, seed, La=4):
    gen = torch.Generator().manual_seed(seed)
    N, c1, D, H, W = shape
    idx = torch.randint(0, La, (N, D, H, W, c1), generator=gen, dtype=torch.uint8)
    y = torch.randn(N, D, H, W, c2, generator=gen) * 3.7
    return idx, y, gen


def _sixteen_class_mask(gen):
    """The mask of test_i8_gram_class_structure_on_a_multi_block_system: a class of 5 voxels, classes of exactly 128 and
    256, three weights in the first volume only."""
    per = 8 * 9 * 10
    others = torch.tensor([1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0])
    rest0 = others[torch.cat([torch.arange(13), torch.randint(0, 13, (per - 5 - 128 - 256 - 13,), generator=gen)])]
    v0 = torch.cat([torch.full((5,), 0.25), torch.full((128,), 12.0), torch.full((256,), 0.5), rest0])
    v0 = v0[torch.randperm(per, generator=gen)]
    v1 = others[torch.cat([torch.arange(13), torch.randint(0, 13, (per - 13,), generator=gen)])]
    return torch.stack([v0, v1[torch.randperm(per, generator=gen)]]).reshape(2, 8, 9, 10)


@pytest.mark.parametrize("with_list", [False, True], ids=["nolist", "16classes"])
def test_uneven_group_edges(ops, with_list):
    """NB 8, NBX 7: the last I group holds block 6 alone, its diagonal group the pairs (6, 6) and (6, 7) only; the ones cell
    (row 864) and the y digits (from row 880) start inside block 6.  With the 16-class list: a class of 5 voxels and
    class changes inside a split."""
    shape, c2 = (2, 32, 8, 9, 10), 32
    idx, y, gen = _data(shape, c2, 55)
    att, cls = None, (None, None, None, 1)
    want = dict(NB=8, NBX=7, npairs=35)
    if with_list:
        att = _sixteen_class_mask(gen)
        cls = ops.att_classes(dev(att))
        assert cls is not None and cls[3] == 16
        sizes = torch.bincount(cls[1].cpu()).tolist()
        assert sizes[0] == 1 and sizes[1] == 2 and sizes[-1] == 1, sizes
        plan = ops.gram_i8_plan(_geom(shape, c2, 3, 1, 1), 16, cls[0].numel())
        assert plan["cps"] > 1 and len(sizes) > plan["nsplit"], (plan, sizes)      # some split holds a class change
    _case(ops, "edges" + ("-16cls" if with_list else ""), shape, c2, 3, idx, y, att, cls, want, 1)


def test_odd_block_count(ops):
    """E = 1072: NB 9, NBX 7 - every group row ends in a J group of one block."""
    shape, c2 = (1, 32, 6, 6, 6), 48
    idx, y, _ = _data(shape, c2, 56)
    _case(ops, "odd NB", shape, c2, 3, idx, y, None, (None, None, None, 1), dict(NB=9, NBX=7, npairs=42), 1)


def test_one_chunk(ops):
    """64 voxels: one half-filled chunk, fewer than the two LDS stages and the two-ahead tables; 133 pairs in 35 groups."""
    shape, c2 = (1, 64, 4, 4, 4), 64
    idx, y, _ = _data(shape, c2, 57)
    _case(ops, "one chunk", shape, c2, 3, idx, y, None, (None, None, None, 1),
          dict(NB=16, NBX=14, npairs=133, nchunks=1, nsplit=1), 1)


def test_k_splits_with_class_changes(ops):
    """128 chunks in 32 splits of 4: three classes of 41, 44 and 43 chunks, so that the last chunk of the first class is
    the first of split 10 and the last of the second the first of split 21 - both flush inside a split."""
    shape, c2 = (4, 32, 16, 16, 16), 32
    idx, y, gen = _data(shape, c2, 58)
    w = torch.cat([torch.full((41 * 128,), 1.0), torch.full((44 * 128,), 2.5), torch.full((43 * 128,), 17.25)])
    att = w[torch.randperm(w.numel(), generator=gen)].reshape(4, 16, 16, 16)
    cls = ops.att_classes(dev(att))
    assert cls is not None and cls[3] == 3 and torch.bincount(cls[1].cpu()).tolist() == [41, 44, 43]
    _case(ops, "K splits", shape, c2, 3, idx, y, att, cls, dict(NB=8, NBX=7, npairs=35, nchunks=128, cps=4, nsplit=32), 1)


@pytest.mark.parametrize("shape,c2,want", [((1, 32, 8, 8, 8), 64, dict(NB=3, NBX=1, npairs=3)),
                                           ((1, 16, 8, 8, 8), 16, dict(NB=1, NBX=1, npairs=1))],
                         ids=["three-pairs", "one-pair"])
def test_single_block_row(ops, shape, c2, want):
    """1^3 layers with one block row: the rule keeps one pair per workgroup (a second I block would be empty)."""
    idx, y, _ = _data(shape, c2, 59 + c2)
    _case(ops, f"one row {want}", shape, c2, 1, idx, y, None, (None, None, None, 1), want, 1)


def test_groups_by_rule_with_cut_splits(ops):
    """64 -> 64, 3^3 at 203 840 voxels: 1593 chunks in 24 splits of 67, the size from which the rule groups.  Every split is
    cut in two (parts of 33 and 34 chunks, the last split of 52 into 26 and 26): the grid is 35 groups x 48."""
    shape, c2 = (1, 64, 56, 56, 65), 64
    idx, y, _ = _data(shape, c2, 60)
    _case(ops, "cut splits", shape, c2, 3, idx, y, None, (None, None, None, 1),
          dict(NB=16, NBX=14, npairs=133, nchunks=1593, cps=67, nsplit=24), 2, want_sub=2)
