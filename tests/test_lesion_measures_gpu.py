"""effq_label_lesion_measures and ``--lesion_measures`` on a real MI355X (-m gpu) against the yardstick of
tests/lesion_measure_ref.py: random nested maps at both connectivities, three spacings and three slice axes, a component
of several candidate tiles beside a small one, more rows than LDS slots and a truncated table, coordinate sums past 2^31,
the form without a truth map, determinism over a dirty workspace, the argument checks, and the score and predict missions
tied back to the files they write.  No tolerance: integers, fp32 bit patterns and file cells are compared exactly."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, nifti, predict, score
from efficientq_amd.hip_ops import get_ops
from efficientq_amd.ops_base import _ptr
from efficientq_amd.ops_measure import label_lesion_measures
from efficientq_amd.ops_score import label_lesions
from tests import lesion_measure_ref as R
from tests.test_lesion_measures_cpu import FLIPPED, LITS, PLAIN, cells, score_args, two_maps, write_score_cases
from tests.test_predict_gpu import _net, _scans, snap_tensor      # noqa: F401 (snap_tensor is a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORDS = _lib.LESION_MEASURE_WORDS
SENTINEL = -77
ERR_ARG, ERR_WORKSPACE = 1, 3           # include/effq_hip.h


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def noise(shape, seed):
    """A map of 0, 1, 2 voxel by voxel: one large component of the liver class and many small ones of both."""
    return np.random.default_rng(seed).choice(np.arange(3, dtype=np.uint8), size=shape, p=(0.62, 0.24, 0.14))


@functools.lru_cache(maxsize=None)
def reference(shape, conn, spacing, axis, seed, with_truth=True):
    pred = noise(shape, seed)
    truth = noise(shape, seed + 1) if with_truth else None
    return (pred, truth) + R.measures(pred, truth, LITS, conn, spacing, axis)


def check_records(got_rows, got_meas, want_rows, want_meas, want_bits, shape, spacing, axis, masks, conn):
    """rows, sums and box against the yardstick; both pairs lie in their component with a <= b, the in-plane one in one
    slice, their E has the bits of the yardstick's maximum, and they are the pair the rule over line ends picks."""
    w = R.weights(spacing)
    for q, mask in enumerate(masks):
        rows, meas = got_rows[q].numpy(), got_meas[q].numpy()
        assert rows.dtype == np.int32 and meas.dtype == np.int64 and meas.shape == (len(rows), WORDS)
        assert np.array_equal(rows, want_rows[q]), q
        assert np.array_equal(meas[:, :9], want_meas[q][:, :9]), q
        lab, _ = R.components(mask, conn)
        flat = lab.ravel()
        for k, m in enumerate(meas):
            for kind in (0, 1):
                a, b = int(m[9 + 2 * kind]), int(m[10 + 2 * kind])
                assert 0 <= a <= b < flat.size and flat[a] == flat[b] == k + 1, (q, k, kind)
                if kind:
                    assert np.unravel_index(a, shape)[axis] == np.unravel_index(b, shape)[axis], (q, k)
                assert R.pair_bits(a, b, shape, w) == int(want_bits[q][k, kind]), (q, k, kind)
            if rows[k, 1] == 1:
                assert m[9] == m[10] == m[11] == m[12] == rows[k, 0]
        assert np.array_equal(meas[:, 9:], want_meas[q][:, 9:]), q


# ---- 1. random maps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", R.SPACINGS)
@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("shape", [(5, 7, 9), (12, 13, 11), (9, 16, 33)])
def test_random_nested_maps_against_the_yardstick(ops, shape, conn, spacing):
    for axis in (0, 1, 2):
        pred, truth, nrows, rows, meas, bits = reference(shape, conn, spacing, axis, sum(shape))
        counts, got_n, got_rows, got_meas = label_lesion_measures(ops, dev(pred), dev(truth), Cf.score_class_lut(LITS), 2,
                                                                  spacing, axis, conn)
        assert counts.dtype == torch.int64 and torch.equal(
            counts, label_lesions(ops, dev(pred), dev(truth), Cf.score_class_lut(LITS), 2, conn).cpu())
        assert got_n.tolist() == nrows.tolist() and min(nrows) >= 1 and max(nrows) > 10
        check_records(got_rows, got_meas, rows, meas, bits, shape, spacing, axis, R.class_planes(pred, truth, LITS), conn)
        assert any((r[:, 1] == 1).any() for r in rows)            # one-voxel components were among them


# ---- 2. several tiles of candidates ---------------------------------------------------------------------------------------------
def ellipsoid():
    """One ellipsoid of more than 1024 line ends along w, and before it in raster order a component of three voxels, so
    that the ellipsoid's candidates start inside a tile of the list."""
    d, h, w = np.ogrid[:40, :40, :48]
    a = (((d - 20) / 14.5) ** 2 + ((h - 20) / 14.5) ** 2 + ((w - 24) / 5.5) ** 2 <= 1.0).astype(np.uint8)
    a[0, 0, 0] = a[0, 0, 1] = a[0, 1, 1] = 1
    return a


def test_a_component_of_several_candidate_tiles_beside_a_small_one(ops):
    a = ellipsoid()
    shape, classes, axis = a.shape, ((1,),), 0
    big = R.components(a, 26)[0] == 2
    assert R.line_ends(big, axis).sum() > 1024 and R.line_ends(a.astype(bool) & ~big, axis).sum() == 3
    pairs = {}
    for spacing in (R.SPACINGS[0], R.SPACINGS[1]):
        nrows, rows, meas, bits = R.measures(a, a, classes, 26, spacing, axis)
        _, got_n, got_rows, got_meas = label_lesion_measures(ops, dev(a), dev(a), [0, 1] + [0] * 254, 1, spacing, axis)
        assert got_n.tolist() == nrows.tolist() == [2, 2]
        check_records(got_rows, got_meas, rows, meas, bits, shape, spacing, axis, [a != 0, a != 0], 26)
        assert got_rows[0][:, 2].tolist() == got_rows[0][:, 1].tolist()                 # a map against itself
        pairs[spacing] = got_meas[0][1, 9:13].tolist()
    # unit spacing: every E is an integer, and the maximum is the one over all voxel pairs, exactly
    brute = R.farthest_brute(big, R.weights(R.SPACINGS[0]), axis)
    for kind in (0, 1):
        e = R.pair_bits(*pairs[R.SPACINGS[0]][2 * kind:2 * kind + 2], shape, R.weights(R.SPACINGS[0]))
        assert e == int(np.array(brute[kind][0]).view(np.uint32))
        assert float(brute[kind][0]) == int(brute[kind][0])
    # at (0.7, 0.7, 2.5) mm the farthest pair lies along w, not in the (d, h) plane
    assert pairs[R.SPACINGS[0]][:2] != pairs[R.SPACINGS[1]][:2]
    (p0, q0), (p1, q1) = ([np.unravel_index(v, shape) for v in pairs[s][:2]] for s in R.SPACINGS[:2])
    assert abs(q0[2] - p0[2]) < 6 < abs(q1[2] - p1[2])


# ---- 3. more rows than slots, and truncation -----------------------------------------------------------------------------------
def isolated():
    a = np.zeros((16, 16, 32), np.uint8)
    d, h, w = np.ogrid[:16, :16, :32]
    a[(d % 2 == 0) & ((h + w) % 2 == 0)] = 1          # 2048 voxels, none a face neighbour of another
    return a


def raw_call(ops, pred, truth, lut, Cc, shape, conn, weights, axis, max_rows, counts, nrows, rows, meas, ws=None,
             ws_bytes=None):
    D, H, W = shape
    if ws is None:
        ws = torch.empty(max(16, ops.lib.effq_label_lesion_measures_ws_bytes(Cc, Cc * (1 if truth is None else 2), D, H, W,
                                                                            max(max_rows, 1))), dtype=torch.uint8, device=DEV)
    rc = ops.lib.effq_label_lesion_measures(
        None if pred is None else _ptr(pred), None if truth is None else _ptr(truth), Cc, D, H, W,
        None if lut is None else (C.c_uint16 * 256)(*lut), conn, *weights, axis, max_rows,
        None if counts is None else _ptr(counts), None if nrows is None else _ptr(nrows),
        None if rows is None else _ptr(rows), None if meas is None else _ptr(meas), _ptr(ws),
        ws.numel() if ws_bytes is None else ws_bytes, ops.stream)
    torch.cuda.synchronize()
    return rc


def sentinels(Cc, P, cap):
    return (torch.full((Cc, 4), SENTINEL, dtype=torch.int64, device=DEV), torch.full((P,), SENTINEL, dtype=torch.int64, device=DEV),
            torch.full((P, cap, 3), SENTINEL, dtype=torch.int32, device=DEV),
            torch.full((P, cap, WORDS), SENTINEL, dtype=torch.int64, device=DEV))


def test_more_rows_than_slots_and_a_table_that_does_not_hold_them(ops):
    a = isolated()
    lut, spacing = [0, 1] + [0] * 254, (1.0, 1.0, 1.0)
    nrows, rows, meas, bits = R.measures(a, None, ((1,),), 6, spacing, 1)
    assert nrows.tolist() == [2048]
    _, got_n, got_rows, got_meas = label_lesion_measures(ops, dev(a), None, lut, 1, spacing, 1, connectivity=6)
    assert got_n.tolist() == [2048]
    check_records(got_rows, got_meas, rows, meas, bits, a.shape, spacing, 1, [a != 0], 6)
    # asked for 64 rows first, the call is repeated with room for all
    again = label_lesion_measures(ops, dev(a), None, lut, 1, spacing, 1, connectivity=6, max_rows=64)
    assert torch.equal(again[2][0], got_rows[0]) and torch.equal(again[3][0], got_meas[0])
    # the truncated call itself: the true count, 64 complete records, nothing else written
    counts, n, r, m = sentinels(1, 1, 80)
    w = [float(v) for v in R.weights(spacing)]
    assert raw_call(ops, dev(a), None, lut, 1, a.shape, 6, w, 1, 64, None, n, r[:, :64], m[:, :64]) == _lib.EFFQ_OK
    assert n.tolist() == [2048]
    assert np.array_equal(r[0, :64].cpu().numpy(), rows[0][:64]) and np.array_equal(m[0, :64].cpu().numpy(), meas[0][:64])
    assert (r[0, 64:] == SENTINEL).all() and (m[0, 64:] == SENTINEL).all()


# ---- 4. sums past 2^31 -----------------------------------------------------------------------------------------------------------
def test_a_full_mask_whose_sums_pass_two_to_the_31(ops):
    D, H, W = shape = (128, 256, 400)
    S = D * H * W
    full = torch.ones(shape, dtype=torch.uint8, device=DEV)
    for axis, planar in ((0, 255 ** 2 + 399 ** 2), (1, 127 ** 2 + 399 ** 2)):
        _, n, rows, meas = label_lesion_measures(ops, full, None, [0, 1] + [0] * 254, 1, (1.0, 1.0, 1.0), axis)
        assert n.tolist() == [1] and rows[0].tolist() == [[0, S, 0]]
        m = meas[0][0].tolist()
        assert m[0:3] == [S * (D - 1) // 2, S * (H - 1) // 2, S * (W - 1) // 2] and max(m[0:3]) > 2 ** 31
        assert m[3:9] == [0, 0, 0, D - 1, H - 1, W - 1]
        p, q = (np.unravel_index(v, shape) for v in m[9:11])
        assert m[9] <= m[10] and all({int(x), int(y)} == {0, e - 1} for x, y, e in zip(p, q, shape))     # opposite corners
        assert sum((int(x) - int(y)) ** 2 for x, y in zip(p, q)) == 127 ** 2 + 255 ** 2 + 399 ** 2
        p, q = (np.unravel_index(v, shape) for v in m[11:13])
        assert m[11] <= m[12] and p[axis] == q[axis]
        assert sum((int(x) - int(y)) ** 2 for x, y in zip(p, q)) == planar


def test_a_component_with_more_tile_pairs_than_one_launch_may_take_is_not_searched(ops):
    # a 3-D checkerboard hangs together at 26-connectivity and every voxel of it ends a line: 6.5e6 line ends, 25600
    # tiles, 3.3e8 tile pairs against the bound of 2^26
    D, H, W = shape = (128, 256, 400)
    d, h, w = (torch.arange(n, device=DEV).view(v) for n, v in zip(shape, ((-1, 1, 1), (1, -1, 1), (1, 1, -1))))
    board = ((d + h + w) % 2 == 0).to(torch.uint8).contiguous()
    tiles = -(-(D * H * W // 2) // 256)
    assert tiles * (tiles + 1) // 2 > _lib.LESION_MEASURE_MAX_TILE_PAIRS
    lut = [0, 1] + [0] * 254
    _, n, r, m = sentinels(1, 1, 2)
    assert raw_call(ops, board, None, lut, 1, shape, 26, [1.0, 1.0, 1.0], 0, 2, None, n, r, m) == _lib.EFFQ_OK
    S = D * H * W // 2
    assert n.tolist() == [1] and r[0, 0].tolist() == [0, S, 0]
    assert m[0, 0, :9].tolist() == [S * (D - 1) // 2, S * (H - 1) // 2, S * (W - 1) // 2, 0, 0, 0, D - 1, H - 1, W - 1]
    assert m[0, 0, 9:].tolist() == [-1, -1, -1, -1]                      # not searched, and said so
    assert (r[0, 1] == SENTINEL).all() and (m[0, 1] == SENTINEL).all()
    with pytest.raises(_lib.EffqError) as e:
        label_lesion_measures(ops, board, None, lut, 1, (1.0, 1.0, 1.0), 0)
    assert "pairs of tiles" in str(e.value) and "not searched" in str(e.value)


# ---- 5. without a truth map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7, 9), (9, 16, 33)])
def test_without_a_truth_map_the_planes_are_the_predicted_ones_also_off_alignment(ops, shape):
    # (5, 7, 9): S % 4 = 3, the tail of the vector path of k_label_bits; the shifted map takes its scalar path
    S = int(np.prod(shape))
    pred, truth = noise(shape, 5), noise(shape, 6)
    lut = Cf.score_class_lut(LITS)
    _, n2, rows2, meas2 = label_lesion_measures(ops, dev(pred), dev(truth), lut, 2, R.SPACINGS[1], 1)
    holder = torch.zeros(S + 1, dtype=torch.uint8, device=DEV)
    shifted = holder[1:].view(shape)                    # one byte off a 4-byte boundary
    shifted.copy_(dev(pred))
    assert shifted.data_ptr() % 4 == 1 and shifted.is_contiguous()
    for p in (dev(pred), shifted):
        counts, n, rows, meas = label_lesion_measures(ops, p, None, lut, 2, R.SPACINGS[1], 1)
        assert counts is None and n.tolist() == n2[:2].tolist() and len(rows) == len(meas) == 2
        for q in range(2):
            assert torch.equal(rows[q][:, :2], rows2[q][:, :2]) and not rows[q][:, 2].any() and rows2[q][:, 2].any()
            assert torch.equal(meas[q], meas2[q])


# ---- 6. determinism -------------------------------------------------------------------------------------------------------------
def test_a_workspace_full_of_ones_gives_the_same_bits_twice(ops):
    a = ellipsoid()
    pred, truth = dev(a), dev(np.roll(a, 3, 2))
    lut = [0, 1] + [0] * 254
    first = label_lesion_measures(ops, pred, truth, lut, 1, R.SPACINGS[2], 2)
    for _ in range(2):
        ops._workspace("lesion_measures", 1).fill_(1)
        got = label_lesion_measures(ops, pred, truth, lut, 1, R.SPACINGS[2], 2)
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])
        assert all(torch.equal(x, y) for x, y in zip(got[2] + got[3], first[2] + first[3]))


# ---- 7. bad arguments -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_their_code_and_leave_every_output_as_it_was(ops):
    shape = (5, 7, 9)
    pred, truth = dev(noise(shape, 1)), dev(noise(shape, 2))
    lut, w = Cf.score_class_lut(LITS), [1.0, 1.0, 4.0]
    query = ops.lib.effq_label_lesion_measures_ws_bytes
    good = dict(pred=pred, truth=truth, lut=lut, Cc=2, shape=shape, conn=26, weights=w, axis=0, max_rows=16)
    ws = torch.empty(query(2, 4, *shape, 16), dtype=torch.uint8, device=DEV)
    assert ws.numel() > 0 and ws.numel() % 16 == 0

    def refused(code, nulls=(), ws_bytes=None, **over):
        kw = dict(good, **over)
        out = dict(zip(("counts", "nrows", "rows", "meas"), sentinels(kw["Cc"] if 0 < kw["Cc"] <= 8 else 1, 4, 16)))
        passed = {k: (None if k in nulls else v) for k, v in out.items()}
        assert raw_call(ops, ws=ws, ws_bytes=ws_bytes, **kw, **passed) == code, (over, nulls)
        assert all((t == SENTINEL).all() for t in out.values()), (over, nulls)
    big = (5, 7, 4097)
    for over in (dict(axis=3), dict(axis=-1), dict(weights=[1.0, 0.0, 1.0]), dict(weights=[-1.0, 1.0, 1.0]),
                 dict(weights=[1.0, float("nan"), 1.0]), dict(weights=[1.0, 1.0, float("inf")]), dict(max_rows=0),
                 dict(max_rows=-4), dict(conn=18), dict(Cc=0), dict(Cc=9), dict(shape=(0, 7, 9)), dict(pred=None),
                 dict(lut=None), dict(lut=[0, 1, 4] + [0] * 253), dict(shape=big)):
        refused(ERR_ARG, **over)
    for null in ("counts", "nrows", "rows", "meas"):
        refused(ERR_ARG, nulls=(null,))
    refused(ERR_WORKSPACE, ws_bytes=ws.numel() - 1)
    assert query(2, 4, *big, 16) == 0 and query(2, 4, 4097, 3, 3, 16) == 0 and query(2, 4, 3, 4097, 3, 16) == 0
    assert query(2, 4, *shape, 0) == 0 and query(0, 0, *shape, 16) == 0 and query(9, 18, *shape, 16) == 0
    assert query(2, 3, *shape, 16) == 0 and query(2, 4, 0, 7, 9, 16) == 0 and query(8, 16, 512, 512, 512, 16) == 0
    assert query(2, 2, *shape, 16) > 0
    # the same arguments, untouched, are served: the checks refused nothing else
    out = sentinels(2, 4, 16)
    assert raw_call(ops, ws=ws, **good, **dict(zip(("counts", "nrows", "rows", "meas"), out))) == _lib.EFFQ_OK
    assert (out[1] > 0).all()
    # and a null counts is fine without a truth map
    out = sentinels(2, 2, 16)
    assert raw_call(ops, ws=ws, **dict(good, truth=None), counts=None, nrows=out[1], rows=out[2], meas=out[3]) == _lib.EFFQ_OK
    with pytest.raises(_lib.EffqError):
        label_lesion_measures(ops, pred, truth, lut, 2, (1.0, 1.0, 1.0), 3)
    with pytest.raises(_lib.EffqError):
        label_lesion_measures(ops, pred, truth, lut, 2, (1.0, 0.0, 1.0), 0)


# ---- 8. the missions ------------------------------------------------------------------------------------------------------------
def test_score_writes_the_tables_of_the_yardstick(ops, tmp_path):
    root = str(tmp_path)
    cases = {"b": two_maps(1, (7, 9, 8)) + (FLIPPED,), "a": two_maps(2, (8, 8, 10)) + (PLAIN,)}
    write_score_cases(root, cases)
    score.run(score_args(root, "plain"), ops=ops)
    score.run(score_args(root, "with", "--lesion_measures"), ops=ops)
    for name in ("scores.csv", "summary.csv"):
        with open(os.path.join(root, "plain", name), "rb") as f, open(os.path.join(root, "with", name), "rb") as g:
            assert f.read() == g.read()
    want, diams = [], []
    for sn, axis in (("a", 2), ("b", 0)):               # b: flipped and anisotropic, its slices are stacked along d
        pred, truth, _ = cases[sn]
        head = nifti.read_geometry(os.path.join(root, "pred", f"{sn}.nii.gz"))
        spacing = tuple(float(v) for v in head["spacing"])
        _, rows, meas, _ = R.measures(pred, truth, LITS, 26, spacing, axis)
        c, d = R.expected_lesions(sn, LITS, True, rows, meas, pred.shape, spacing, head["affine"], axis)
        want, diams = want + c, diams + d
    got = cells(os.path.join(root, "with", "lesions.csv"))
    assert got[0] == list(R.COLUMNS) and got[1:] == want and len(want) > 12
    detect = cells(os.path.join(root, "with", "lesion_detect.csv"))
    assert detect[1:] == R.expected_detect(LITS, want, diams)


def test_predict_writes_the_lesions_of_the_map_it_writes(ops, snap_tensor, tmp_path):
    root, out = str(tmp_path), str(tmp_path / "seg")
    lst = _scans(root, ["a"])
    args, _ = _net()
    for k, v in dict(src_list=lst, out_dir=out, patch_size="32,32,32", prep_spacing=None, prep_mask="nonzero",
                     resume=os.path.join(snap_tensor[0], "state_in_fp.pkl"), merge_type=None, lesion_measures=True).items():
        setattr(args, k, v)
    predict.run(args, window_batch=1)
    got, _ = nifti.read_nifti(os.path.join(out, "a.nii.gz"))
    head = nifti.read_geometry(os.path.join(root, "src", "a.nii.gz"))         # the scan's: the map is on its grid
    spacing = tuple(float(v) for v in head["spacing"])
    assert spacing == (1.0, 1.0, 2.0)
    _, rows, meas, _ = R.measures(got, None, LITS, 26, spacing, 2)
    full, _ = R.expected_lesions("a", LITS, False, rows, meas, got.shape, spacing, head["affine"], 2)
    table = cells(os.path.join(out, "lesions.csv"))
    assert table[0] == [k for k in R.COLUMNS if k != "overlap"]
    print("lesions of the predicted map per plane:", [len(r) for r in rows])
    assert table[1:] == [r[:9] + r[10:] for r in full] and full
