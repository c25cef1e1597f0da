"""effq_label_clean and effq_label_tallies on a real MI355X (-m gpu), bit for bit against the numpy restatement of
tests/label_clean_ref.py: everything is integer, so no tolerance appears anywhere.  The labelling tile is 8 x 8 x 32, and
the shapes are the smallest that cross it in every way."""
import ctypes as C

import numpy as np
import pytest
import torch

from efficientq_amd import _lib
from efficientq_amd.hip_ops import get_ops
from tests import label_clean_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def _clean(ops, a, rules, conn, inplace=False):
    m = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    before = m.clone()
    out, stats = ops.label_clean(m, rules, conn, out=m if inplace else None)
    assert out.dtype == torch.uint8 and out.shape == m.shape and stats.dtype == torch.int64
    assert stats.shape == (len(rules), 2) and (inplace or torch.equal(m, before))
    return out.cpu().numpy(), stats.cpu().numpy()


def _check(ops, a, rules, conn):
    got, stats = _clean(ops, a, rules, conn)
    want, wstats = R.clean(a, rules, conn)
    assert np.array_equal(got, want), f"{int((got != want).sum())} voxels differ for {rules} at {conn}"
    assert np.array_equal(stats, wstats), f"stats {stats.tolist()}, want {wstats.tolist()} for {rules} at {conn}"
    return got, stats


def _random_map(shape, seed, density=0.35):
    g = np.random.default_rng(seed)
    fg = g.random(shape) < density
    return np.where(fg, g.choice(np.array([1, 2, 4], dtype=np.uint8), size=shape), 0).astype(np.uint8)


def _fill(a, box, count, value):
    """The first `count` voxels of the box (three slices) in raster order get `value`: one 6-connected component."""
    sub = a[box]
    flat = sub.reshape(-1).copy()
    assert count <= flat.size and not flat.any()
    flat[:count] = value
    a[box] = flat.reshape(sub.shape)


# ---- random maps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [(1,), (2, 4)])
@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("shape", [(1, 1, 1), (8, 8, 32), (9, 17, 70), (3, 5, 33), (17, 9, 65)])
def test_random_maps_match_the_restatement(ops, shape, conn, labels):
    a = _random_map(shape, sum(shape) + conn)
    if shape == (1, 1, 1):
        a[...] = labels[0]
    for rule in [(labels, "largest", 0, 0), (labels, "min", 1, 0), (labels, "min", 2, 3), (labels, "min", 7, 0)]:
        _, stats = _check(ops, a, [rule], conn)
        assert stats[0, 0] >= 1
    if len(a.reshape(-1)) > 1:      # large and small components: both ops have something to do and something to keep
        sizes = R.component_sizes(R.first_voxels(np.isin(a, labels), conn))[1]
        assert sizes.max() >= 7 > sizes.min() and len(sizes) > 3


# ---- ties -------------------------------------------------------------------------------------------------------------
def test_of_equal_largest_components_the_one_with_the_least_first_voxel_stays(ops):
    cube = lambda d, h, w: (slice(d, d + 2), slice(h, h + 2), slice(w, w + 2))
    for conn in (6, 26):
        # two of 8 voxels in different tiles; the one that comes first in raster order lies further along w
        a = np.zeros((20, 20, 70), dtype=np.uint8)
        a[cube(2, 10, 50)] = 1
        a[cube(12, 3, 5)] = 1
        a[17, 1, 1:4] = 1                        # and a smaller one
        got, stats = _check(ops, a, [((1,), "largest", 0, 0)], conn)
        assert got[cube(2, 10, 50)].all() and got.sum() == 8 and stats.tolist() == [[3, 11]]
        # three of equal size
        a[cube(17, 17, 66)] = 1
        got, stats = _check(ops, a, [((1,), "largest", 0, 7)], conn)
        assert (got[cube(2, 10, 50)] == 1).all() and (got == 1).sum() == 8 and (got == 7).sum() == 19
        assert stats.tolist() == [[4, 19]]
        # a later, strictly larger component wins
        a[18, 8, 2:11] = 1
        got, stats = _check(ops, a, [((1,), "largest", 0, 0)], conn)
        assert got[18, 8, 2:11].all() and got.sum() == 9 and stats.tolist() == [[5, 27]]


# ---- the threshold ----------------------------------------------------------------------------------------------------
def _threshold_map():
    """Components of 100, 101 and 102 voxels and one of 50 + 51 voxels that meet in one corner, at the corner of four
    tiles.  The one of 100 snakes through three tiles along each axis."""
    a = np.zeros((20, 20, 70), dtype=np.uint8)
    a[0, 0, 0:67] = 1                            # along w: tiles 0, 1, 2
    a[0, 1:18, 66] = 1                           # along h: tiles 0, 1, 2
    a[1:17, 17, 66] = 1                          # along d: tiles 0, 1, 2
    assert a.sum() == 100
    _fill(a, (slice(4, 9), slice(2, 7), slice(10, 15)), 101, 1)
    _fill(a, (slice(12, 19), slice(8, 13), slice(28, 36)), 102, 1)
    _fill(a, (slice(6, 8), slice(3, 8), slice(27, 32)), 50, 1)            # ends at (7, 7, 31)
    _fill(a, (slice(8, 11), slice(8, 12), slice(32, 37)), 51, 1)          # starts at (8, 8, 32)
    return a


def test_a_component_of_exactly_n_voxels_stays_and_one_of_n_minus_1_goes(ops):
    a = _threshold_map()
    n = 101
    got, stats = _check(ops, a, [((1,), "min", n, 0)], 26)
    assert stats.tolist() == [[4, 100]] and not got[0].any() and not got[:, 17, 66].any()
    assert got.sum() == 101 + 102 + 101 and got[7, 7, 31] == 1 and got[8, 8, 32] == 1
    got, stats = _check(ops, a, [((1,), "min", n, 0)], 6)                 # the corner no longer joins the two
    assert stats.tolist() == [[5, 201]] and got.sum() == 101 + 102 and got[7, 7, 31] == 0 and got[8, 8, 32] == 0
    for conn in (6, 26):
        _check(ops, a, [((1,), "min", n - 1, 0)], conn)
        _check(ops, a, [((1,), "min", n + 1, 0)], conn)
        _check(ops, a, [((1,), "min", n + 2, 5)], conn)


# ---- order --------------------------------------------------------------------------------------------------------------
def test_rules_apply_in_the_order_given(ops):
    a = np.zeros((10, 12, 40), dtype=np.uint8)
    a[2:6, 2:8, 3:30] = 1
    a[8, 10, 36:39] = 2                          # a speck of label 2, far from the body
    first = [((2,), "min", 5, 1), ((1,), "largest", 0, 0)]
    one, s1 = _check(ops, a, first, 26)
    two, s2 = _check(ops, a, first[::-1], 26)
    assert not np.array_equal(one, two)
    assert one[8, 10, 37] == 0 and two[8, 10, 37] == 1                  # relabelled and then dropped / kept
    assert s1.tolist() == [[1, 3], [2, 3]] and s2.tolist() == [[1, 0], [1, 3]]


# ---- in place -----------------------------------------------------------------------------------------------------------
def test_in_place_gives_the_bits_of_the_out_of_place_call(ops):
    a = _random_map((9, 17, 70), 5)
    rules = [((1, 2), "largest", 0, 0), ((4,), "min", 4, 1), ((1,), "min", 3, 2)]
    for conn in (6, 26):
        out, s1 = _clean(ops, a, rules, conn)
        inp, s2 = _clean(ops, a, rules, conn, inplace=True)
        assert np.array_equal(out, inp) and np.array_equal(s1, s2)
        want, wst = R.clean(a, rules, conn)
        assert np.array_equal(out, want) and np.array_equal(s1, wst)


# ---- nothing to do --------------------------------------------------------------------------------------------------------
def test_an_empty_mask_and_a_single_component_change_nothing(ops):
    a = np.zeros((9, 9, 40), dtype=np.uint8)
    a[1:8, 2:9, 5:38] = 2
    for conn in (6, 26):
        got, stats = _check(ops, a, [((3,), "largest", 0, 0), ((3, 7), "min", 50, 0)], conn)
        assert np.array_equal(got, a) and stats.tolist() == [[0, 0], [0, 0]]
        got, stats = _check(ops, a, [((2,), "largest", 0, 0), ((2,), "min", 7 * 7 * 33, 0)], conn)
        assert np.array_equal(got, a) and stats.tolist() == [[1, 0], [1, 0]]


# ---- many roots -----------------------------------------------------------------------------------------------------------
def test_one_large_component_among_thousands_of_specks(ops):
    shape = (64, 96, 160)
    g = np.random.default_rng(11)
    a = (g.random(shape) < 0.004).astype(np.uint8)
    a[10:50, 20:70, 30:130] = 0
    a[12:48, 22:68, 32:128] = 1
    names = R.first_voxels(a == 1, 26)           # once for both rules
    ids, sizes = R.component_sizes(names)
    assert len(ids) > 2000 and sizes.max() == 36 * 46 * 96 and (sizes == 2).sum() > 10
    body = names == ids[np.argmax(sizes)]
    got, stats = _clean(ops, a, [((1,), "largest", 0, 0)], 26)
    assert np.array_equal(got, body.astype(np.uint8))
    assert stats.tolist() == [[len(ids), int((a == 1).sum() - body.sum())]]
    got, stats = _clean(ops, a, [((1,), "min", 2, 9)], 26)
    single = np.isin(names, ids[sizes < 2])
    assert np.array_equal(got, np.where(single, 9, a).astype(np.uint8))
    assert stats.tolist() == [[len(ids), int(single.sum())]]


# ---- bad arguments ----------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_their_code_and_write_nothing(ops):
    D, H, W = 4, 5, 6
    lib = ops.lib
    m = torch.ones(D, H, W, dtype=torch.uint8, device=DEV)
    out = torch.full((D, H, W), 0xA5, dtype=torch.uint8, device=DEV)
    stats = torch.full((2, 2), -77, dtype=torch.int64, device=DEV)
    need = lib.effq_label_clean_ws_bytes(D, H, W)
    assert need >= 9 * D * H * W
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(R_=2, sets=None, rules=None, conn=26, dims=(D, H, W), null=None, ws_bytes=need):
        s = (C.c_uint8 * (256 * 8))()
        s[1] = s[256 + 2] = 1
        for k, v in (sets or {}).items():
            s[k] = v
        r = (C.c_longlong * 24)(*([0, 0, 0, 1, 3, 0] + [0] * 18))
        for k, v in (rules or {}).items():
            r[k] = v
        a = dict(inp=ptr(m), sets=s, rules=r, out=ptr(out), stats=ptr(stats), ws=ptr(ws))
        if null:
            a[null] = None
        rc = lib.effq_label_clean(a["inp"], *dims, conn, R_, a["sets"], a["rules"], a["out"], a["stats"], a["ws"],
                                  ws_bytes, ops.stream)
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all()) and bool((stats == -77).all())
        return rc

    ARG, WS = 1, 3
    for name in ("inp", "sets", "rules", "out", "stats", "ws"):
        assert call(null=name) == ARG, name
    assert call(R_=0) == ARG and call(R_=9) == ARG and call(R_=-1) == ARG
    assert call(rules={0: 2}) == ARG and call(rules={3: -1}) == ARG                  # an op other than the two
    assert call(rules={4: 0}) == ARG and call(rules={4: -5}) == ARG                  # N < 1
    assert call(rules={2: -1}) == ARG and call(rules={5: 256}) == ARG                # TO outside 0..255
    assert call(rules={2: 1}) == ARG and call(rules={5: 2}) == ARG                   # TO in its own set
    assert call(sets={0: 1}) == ARG and call(sets={256: 1}) == ARG                   # the value 0 in a mask
    assert call(conn=18) == ARG and call(conn=0) == ARG
    for dims in ((0, H, W), (D, -1, W), (D, H, 0), (2048, 1024, 1024)):
        assert call(dims=dims) == ARG, dims
        assert lib.effq_label_clean_ws_bytes(*dims) == 0
    assert call(ws_bytes=need - 1) == WS and call(ws_bytes=0) == WS
    # and the same call with nothing wrong runs (rule 1 is judged on the map rule 0 left)
    assert lib.effq_label_clean(ptr(m), D, H, W, 26, 2, *_good(), ptr(out), ptr(stats), ptr(ws), need, ops.stream) == 0
    assert bool((out == 1).all()) and stats.cpu().tolist() == [[1, 0], [0, 0]]
    # the wrapper refuses before the library is asked
    for bad in ([], [((1,), "largest", 0, 0)] * 9, [((1,), "biggest", 0, 0)], [((0,), "largest", 0, 0)],
                [((1,), "min", 0, 0)], [((1,), "min", 3, 1)], [((1,), "min", 3, 256)], [((), "largest", 0, 0)]):
        with pytest.raises(_lib.EffqError):
            ops.label_clean(m, bad)
    for bad in (dict(connectivity=18), dict(out=torch.empty(D, H, W + 1, dtype=torch.uint8, device=DEV))):
        with pytest.raises(_lib.EffqError):
            ops.label_clean(m, [((1,), "largest", 0, 0)], **bad)
    with pytest.raises(_lib.EffqError):
        ops.label_clean(m.to(torch.int32), [((1,), "largest", 0, 0)])


def _good():
    s = (C.c_uint8 * 512)()
    s[1] = s[256 + 2] = 1
    return s, (C.c_longlong * 6)(0, 0, 0, 1, 3, 0)


# ---- label_tallies -----------------------------------------------------------------------------------------------------------
SIZES = [7 * 9 * 37, 2 ** 20 + 3]


@pytest.fixture(scope="module")
def cases():
    """Per S: logits 3 x S, a class-id truth and a brats-valued truth map, made once."""
    out = {}
    for S in SIZES + [8 * 9 * 37]:
        g = torch.Generator().manual_seed(S)
        logits = torch.randn(3, S, generator=g)
        ids = torch.randint(0, 3, (S,), generator=g).to(torch.uint8)
        vals = torch.tensor([0, 1, 2, 4], dtype=torch.uint8)[torch.randint(0, 4, (S,), generator=g)]
        out[S] = (logits.to(DEV), ids.to(DEV), vals.to(DEV))
    return out


def _planes(vals, lut):
    bits = torch.tensor(lut, dtype=torch.int64, device=vals.device)[vals.long()]
    return torch.stack([(bits >> c) & 1 for c in range(3)]).to(torch.uint8).contiguous()


@pytest.mark.parametrize("S", SIZES)
def test_label_tallies_of_the_decided_map_are_seg_tallies_bits(ops, cases, S):
    logits, ids, vals = cases[S]
    lut = R.class_lut("argmax", 3)
    pred = ops.seg_labels(logits[None], "argmax", None, torch.uint8)[0]
    got = ops.label_tallies(pred, ids, lut, 3)
    want = ops.seg_tallies(logits, ids, "lits")
    assert got.dtype == torch.int64 and got.shape == (3, 4) and torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy(), R.tallies(pred.cpu().numpy(), ids.cpu().numpy(), lut, 3))
    assert int(got[0].sum()) == S
    lut = R.class_lut("brats", 3)
    planes = _planes(vals, lut)
    for fuse in ("agg", "con"):
        pred = ops.seg_labels(logits[None], "brats", fuse, torch.uint8)[0]
        got = ops.label_tallies(pred, vals, lut, 3)
        assert torch.equal(got, ops.seg_tallies(logits, planes, "brats", fuse)), fuse
        assert np.array_equal(got.cpu().numpy(), R.tallies(pred.cpu().numpy(), vals.cpu().numpy(), lut, 3))


@pytest.mark.parametrize("S", SIZES + [8 * 9 * 37])
def test_label_tallies_with_planes_truth_equal_the_map_form(ops, cases, S):
    logits, _, vals = cases[S]
    lut = R.class_lut("brats", 3)
    planes = _planes(vals, lut)
    pred = ops.seg_labels(logits[None], "brats", "agg", torch.uint8)[0]
    got = ops.label_tallies(pred, planes, lut, 3)
    assert torch.equal(got, ops.label_tallies(pred, vals, lut, 3))
    assert np.array_equal(got.cpu().numpy(), R.tallies(pred.cpu().numpy(), planes.cpu().numpy(), lut, 3))
    # a plane counts when it is non-zero, whatever its value; a view that is not 4-B aligned takes the other path
    got = ops.label_tallies(pred, planes * 3, lut, 3)
    assert torch.equal(got, ops.label_tallies(pred, vals, lut, 3))
    if S % 4 == 0:
        assert torch.equal(ops.label_tallies(pred[1:], vals[1:], lut, 3),
                           torch.from_numpy(R.tallies(pred[1:].cpu().numpy(), vals[1:].cpu().numpy(), lut, 3)).to(DEV))


def test_label_tallies_refuses_what_it_cannot_count(ops):
    p = torch.zeros(4, 5, dtype=torch.uint8, device=DEV)
    lut = R.class_lut("argmax", 3)
    for bad in (dict(truth=p[:3]), dict(truth=p.to(torch.int32)), dict(lut=lut[:255]), dict(lut=[8] * 256),
                dict(C_=0), dict(C_=9), dict(truth=torch.zeros(2, 4, 5, dtype=torch.uint8, device=DEV))):
        kw = dict(truth=p, lut=lut, C_=3)
        kw.update(bad)
        with pytest.raises(_lib.EffqError):
            ops.label_tallies(p, **kw)
    short = torch.zeros(16, dtype=torch.uint8, device=DEV)
    counts = torch.full((3, 4), -7, dtype=torch.int64, device=DEV)
    rc = ops.lib.effq_label_tallies(C.c_void_p(p.data_ptr()), C.c_void_p(p.data_ptr()), 0, 3, 20,
                                    (C.c_uint16 * 256)(*lut), C.c_void_p(counts.data_ptr()),
                                    C.c_void_p(short.data_ptr()), 16, ops.stream)
    torch.cuda.synchronize()
    assert rc == 3 and bool((counts == -7).all())
