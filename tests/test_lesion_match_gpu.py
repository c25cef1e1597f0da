"""The lesion pairs on a real MI355X (-m gpu): effq_seg_lesion_match pair for pair against ref_pairs of
tests/lesion_match_ref.py, every call twice on a workspace filled with 0xFF, its shared outputs against
seg_lesion_table's; the hazards of the kernel one by one (a key from many workgroups, many keys per wave and workgroup,
rows above 65535, a full table), the refusals, and the ptq mission with --lesion_match tied back to the maps it writes."""
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, lesion_match as LM
from efficientq_amd.hip_ops import get_ops
from efficientq_amd.nifti import read_nifti
from efficientq_amd.ops_match import seg_lesion_match
from tests.lesion_match_ref import ref_pairs, ref_scores
from tests.test_seg_eval_cpu import write_dataset
from tests.test_seg_labels_gpu import _logits, merge_basic, pred_lits
from tests.test_seg_lesions_gpu import _blocky

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARG, WS = 1, 3


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _match_twice(ops, x, lab, task, fuse, max_rows=None, max_pairs=None):
    """seg_lesion_match on a workspace filled with 0xFF, twice: the same bits both times, and the shared outputs are
    seg_lesion_table's."""
    seg_lesion_match(ops, x, lab, task, fuse, max_rows, max_pairs)          # sizes the workspace
    ops._ws["cc"].fill_(0xFF)
    one = seg_lesion_match(ops, x, lab, task, fuse, max_rows, max_pairs)
    ops._ws["cc"].fill_(0xFF)
    two = seg_lesion_match(ops, x, lab, task, fuse, max_rows, max_pairs)
    Cc = x.shape[0]
    for a, b in zip(one[:2], two[:2]):
        assert torch.equal(a, b)
    for k in (2, 3):
        assert len(one[k]) == len(two[k]) and all(torch.equal(a, b) for a, b in zip(one[k], two[k]))
    counts, nrows, rows, pairs = one
    tc, tn, tr = ops.seg_lesion_table(x, lab, task, fuse)
    assert counts.dtype == torch.int64 and counts.shape == (Cc, 4) and torch.equal(counts, tc)
    assert torch.equal(nrows, tn) and len(rows) == 2 * Cc and all(torch.equal(a, b) for a, b in zip(rows, tr))
    assert len(pairs) == Cc and all(p.dtype == torch.int32 and p.dim() == 2 and p.shape[1] == 3 for p in pairs)
    return counts, nrows, rows, [p.numpy().astype(np.int64) for p in pairs]


def _check_case(ops, x, lab, task, fuse, pred, gt):
    _, nrows, rows, pairs = _match_twice(ops, x, lab, task, fuse)
    Cc = x.shape[0]
    for c in range(Cc):
        a, b, want = ref_pairs(pred[c], gt[c])
        assert np.array_equal(pairs[c], want), f"class {c}: {len(pairs[c])} pairs, the reference has {len(want)}"
        assert np.array_equal(rows[Cc + c].numpy()[:, 1], a) and np.array_equal(rows[c].numpy()[:, 1], b)
        assert pairs[c][:, 2].sum() == (np.asarray(pred[c], bool) & np.asarray(gt[c], bool)).sum()
    return pairs


def _planes(pred, gt):
    """Logits and label of the sigmoid decision whose masks are the given ones: C independent channels."""
    x = torch.where(torch.as_tensor(np.asarray(pred)).bool(), 4.0, -4.0).float().contiguous().to(DEV)
    return x, torch.as_tensor(np.asarray(gt)).to(torch.uint8).contiguous().to(DEV)


def _lattice(shape):
    m = np.zeros(shape, np.uint8)
    m[::2, ::2, ::2] = 1
    return m


# ---- seeded random masks --------------------------------------------------------------------------------------------
SHAPE = (12, 20, 40)
RAGGED = (7, 19, 53)                                    # 7049 voxels: no multiple of the workgroup, the scalar mask path


@pytest.mark.parametrize("shape", [SHAPE, RAGGED])
@pytest.mark.parametrize("fuse", [None, "agg", "con"])
def test_sigmoid_pairs_equal_the_reference(ops, fuse, shape):
    assert (RAGGED[0] * RAGGED[1] * RAGGED[2]) % 256 != 0
    x = _logits(ops, 1, 3, shape, 53, sigmoid=True)[0]
    big = tuple(-(-s // 4) * 4 for s in shape)
    lab = _blocky(big, 2, 63, channels=3)[:, :shape[0], :shape[1], :shape[2]].contiguous().to(DEV)
    hard = merge_basic((torch.sigmoid(x[None]) >= 0.5).int(), fuse)[0].cpu().numpy()
    pairs = _check_case(ops, x, lab, "brats", fuse, hard, lab.cpu().numpy())
    assert all(len(p) >= 1 for p in pairs)          # masks this dense are a giant component and its dust


@pytest.mark.parametrize("shape", [SHAPE, RAGGED])
def test_argmax_pairs_equal_the_reference(ops, shape):
    x = _logits(ops, 1, 3, shape, 33, sigmoid=False)[0]
    big = tuple(-(-s // 4) * 4 for s in shape)
    lab = _blocky(big, 3, 43)[:shape[0], :shape[1], :shape[2]].contiguous().to(DEV)
    pred, labn = pred_lits(x[None])[0].cpu().numpy(), lab.cpu().numpy()
    _check_case(ops, x, lab, "lits", None, [pred == c for c in range(3)], [labn == c for c in range(3)])


def test_random_blobs_at_several_densities(ops):
    shape = (9, 21, 37)
    rng = np.random.default_rng(5)
    gt = np.stack([rng.random(shape) < d for d in (0.03, 0.12, 0.3)])
    pred = np.stack([(rng.random(shape) < d) | (g & (rng.random(shape) < 0.6)) for d, g in zip((0.05, 0.1, 0.35), gt)])
    x, lab = _planes(pred, gt)
    _check_case(ops, x, lab, "brats", None, pred, gt)


# ---- the hazards ----------------------------------------------------------------------------------------------------
def test_one_key_from_many_workgroups(ops):
    """Two overlapping boxes in 65 x 128 x 130 = 1 081 600 voxels, more than the 4096 x 256 of one grid-stride trip: one
    pair whose count is the intersection, summed over every workgroup that meets it.  The second channel is the
    complements: one pair again."""
    D, H, W = 65, 128, 130
    assert D * H * W > 4096 * 256
    gt = np.zeros((2, D, H, W), np.uint8)
    pred = np.zeros_like(gt)
    gt[0, 3:60, 10:120, 5:100] = 1
    pred[0, 20:65, 0:90, 40:130] = 1
    gt[1], pred[1] = 1 - gt[0], 1 - pred[0]
    x, lab = _planes(pred, gt)
    _, nrows, rows, pairs = _match_twice(ops, x, lab, "brats", None)
    inter = 40 * 80 * 60
    assert int((gt[0] & pred[0]).sum()) == inter
    assert nrows.tolist() == [1, 1, 1, 1]
    assert pairs[0].tolist() == [[0, 0, inter]]
    union = int(gt[0].sum()) + int(pred[0].sum()) - inter
    assert pairs[1].tolist() == [[0, 0, D * H * W - union]]


def test_many_keys_per_wave_and_workgroup(ops):
    """The label is the isolated voxels of the stride-2 lattice, the prediction everything: one predicted lesion against
    D/2 H/2 W/2 label lesions, 32 distinct keys in a wave (more than the match rounds) and 64 to 128 in the 256 direct-
    mapped slots of a workgroup, where many collide and go to the table singly."""
    shape = (16, 24, 64)
    gt = _lattice(shape)[None]
    pred = np.ones_like(gt)
    x, lab = _planes(pred, gt)
    _, nrows, _, pairs = _match_twice(ops, x, lab, "brats", None)
    n = 8 * 12 * 32
    assert nrows.tolist() == [1, n]
    assert np.array_equal(pairs[0], np.stack([np.arange(n), np.zeros(n, np.int64), np.ones(n, np.int64)], 1))
    _check_case(ops, x, lab, "brats", None, pred, gt)
    # and the other way round: one label lesion, many predicted ones
    x, lab = _planes(gt, pred)
    _, nrows, _, pairs = _match_twice(ops, x, lab, "brats", None)
    assert np.array_equal(pairs[0], np.stack([np.zeros(n, np.int64), np.arange(n), np.ones(n, np.int64)], 1))


def _raw(ops, x, lab, mode, max_rows, max_pairs, guard=0, fill=-7, ws_fill=0xFF):
    """effq_seg_lesion_match itself on outputs filled with `fill`, `guard` words behind pairs included."""
    Cc, D, H, W = x.shape
    need = ops.lib.effq_seg_lesion_match_ws_bytes(Cc, D, H, W, max_rows, max_pairs)
    assert need > ops.lib.effq_cc_table_ws_bytes(2 * Cc, D, H, W, max_rows) > 0
    ws = torch.full((need,), ws_fill, dtype=torch.uint8, device=DEV)
    out = dict(counts=torch.full((Cc, 4), fill, dtype=torch.int64, device=DEV),
               nrows=torch.full((2 * Cc,), fill, dtype=torch.int64, device=DEV),
               rows=torch.full((2 * Cc, max_rows, 3), fill, dtype=torch.int32, device=DEV),
               npairs=torch.full((Cc,), fill, dtype=torch.int64, device=DEV),
               pairs=torch.full((Cc * max_pairs * 3 + guard,), fill, dtype=torch.int32, device=DEV))
    thresh = ops.sigmoid_threshold() if mode == _lib.SEG_SIGMOID else 0.0
    rc = ops.lib.effq_seg_lesion_match(_ptr(x), _ptr(lab), Cc, D, H, W, mode, 0, thresh, 26, max_rows, max_pairs,
                                       _ptr(out["counts"]), _ptr(out["nrows"]), _ptr(out["rows"]), _ptr(out["npairs"]),
                                       _ptr(out["pairs"]), _ptr(ws), need, ops.stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu() for k, v in out.items()}


def test_rows_above_65535(ops):
    """The stride-2 lattice of 96 x 96 x 64 in both masks: 73 728 lesions and 73 728 pairs (i, i), rows that do not fit
    16 bits.  At the default capacity the class reports -1 and the class beside it is complete; the wrapper asks again
    until all of them are there, in order."""
    shape = (96, 96, 64)
    n = 48 * 48 * 32
    assert n == 73728 > 65535 and n > _lib.LESION_PAIR_ROWS
    lat = _lattice(shape)
    box = np.zeros(shape, np.uint8)
    box[1:9, 1:9, 1:9] = 1
    x, lab = _planes(np.stack([lat, box]), np.stack([lat, box]))
    rc, out = _raw(ops, x, lab, _lib.SEG_SIGMOID, _lib.LESION_TABLE_ROWS, _lib.LESION_PAIR_ROWS, guard=64)
    assert rc == 0
    assert out["npairs"].tolist() == [-1, 1] and out["nrows"].tolist() == [n, 1, n, 1]
    assert out["pairs"][3 * _lib.LESION_PAIR_ROWS:3 * _lib.LESION_PAIR_ROWS + 3].tolist() == [0, 0, 512]
    assert (out["pairs"][-64:] == -7).all()
    _, nrows, rows, pairs = seg_lesion_match(ops, x, lab, "brats")
    assert nrows.tolist() == [n, 1, n, 1] and len(rows[0]) == n
    ids = np.arange(n, dtype=np.int64)
    assert np.array_equal(pairs[0].numpy().astype(np.int64), np.stack([ids, ids, np.ones(n, np.int64)], 1))
    assert pairs[1].tolist() == [[0, 0, 512]]
    # the first voxels of the rows are the lattice in raster order: row i of both planes is the same voxel
    assert np.array_equal(rows[0].numpy()[:, 0], np.flatnonzero(lat.reshape(-1)))


def test_all_to_all_and_a_table_that_is_too_small(ops):
    """The label is the planes h even, the prediction the planes w even: (H/2)(W/2) pairs of D voxels each.  With a
    small max_pairs the class reports -1, nothing is written past the table, and the classes beside it are intact."""
    D, H, W = 6, 32, 48
    d, h, w = np.indices((D, H, W))
    box = np.zeros((D, H, W), np.uint8)
    box[1:4, 2:9, 3:11] = 1
    shifted = np.roll(box, 2, 2)
    gt = np.stack([box, (h % 2 == 0).astype(np.uint8), np.zeros_like(box)])
    pred = np.stack([shifted, (w % 2 == 0).astype(np.uint8), box])
    x, lab = _planes(pred, gt)
    pairs = _check_case(ops, x, lab, "brats", None, pred, gt)
    n = (H // 2) * (W // 2)
    assert len(pairs[1]) == n and (pairs[1][:, 2] == D).all()
    assert np.array_equal(pairs[1][:, :2], np.stack([np.repeat(np.arange(H // 2), W // 2),
                                                    np.tile(np.arange(W // 2), H // 2)], 1))
    assert pairs[0].tolist() == [[0, 0, 3 * 7 * 6]] and len(pairs[2]) == 0
    for cap in (1, 100, n - 1):
        rc, out = _raw(ops, x, lab, _lib.SEG_SIGMOID, 64, cap, guard=4096)
        assert rc == 0
        assert out["npairs"].tolist() == [1, -1, 0], cap
        assert (out["pairs"][3 * cap * 3:] == -7).all(), cap               # the guard band
        assert out["pairs"][:3].tolist() == [0, 0, 3 * 7 * 6], cap
        assert (out["pairs"][3:3 * cap] == -7).all() and (out["pairs"][2 * 3 * cap:3 * 3 * cap] == -7).all(), cap
    rc, out = _raw(ops, x, lab, _lib.SEG_SIGMOID, 64, n, guard=4096)
    assert rc == 0 and out["npairs"].tolist() == [1, n, 0]
    assert np.array_equal(out["pairs"][3 * n:6 * n].view(n, 3).numpy(), pairs[1])
    assert (out["pairs"][9 * n:] == -7).all()
    # the wrapper doubles a capacity that is too small until the class fits
    got = seg_lesion_match(ops, x, lab, "brats", None, None, 3)[3]
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(got, pairs))


# ---- other cases ----------------------------------------------------------------------------------------------------
def test_empty_masks_have_no_pairs(ops):
    shape = (5, 9, 13)
    z, one = np.zeros((1,) + shape, np.uint8), np.ones((1,) + shape, np.uint8)
    for pred, gt in ((z, z), (one, z), (z, one)):
        x, lab = _planes(pred, gt)
        _, nrows, _, pairs = _match_twice(ops, x, lab, "brats", None)
        assert nrows.tolist() == [int(pred.any()), int(gt.any())] and pairs[0].shape == (0, 3)
        rc, out = _raw(ops, x, lab, _lib.SEG_SIGMOID, 4, 4)
        assert rc == 0 and out["npairs"].tolist() == [0] and (out["pairs"] == -7).all()


def test_truncated_rows_leave_the_pairs_complete(ops):
    shape = (9, 21, 37)
    rng = np.random.default_rng(9)
    gt = (rng.random((2,) + shape) < 0.1).astype(np.uint8)
    pred = ((rng.random((2,) + shape) < 0.1) | ((gt > 0) & (rng.random((2,) + shape) < 0.5))).astype(np.uint8)
    x, lab = _planes(pred, gt)
    want = [ref_pairs(pred[c], gt[c]) for c in range(2)]
    npairs = max(len(w[2]) for w in want)
    rc, out = _raw(ops, x, lab, _lib.SEG_SIGMOID, 1, npairs)
    assert rc == 0
    assert out["nrows"].tolist() == [len(want[0][1]), len(want[1][1]), len(want[0][0]), len(want[1][0])]
    assert min(out["nrows"].tolist()) > 1                                    # every plane is truncated to its first row
    for c in range(2):
        assert int(out["npairs"][c]) == len(want[c][2])
        got = out["pairs"][3 * npairs * c:3 * npairs * c + 3 * len(want[c][2])].view(-1, 3).numpy()
        assert np.array_equal(got, want[c][2]), c
    assert out["rows"][:, 0, 1].tolist() == [int(want[0][1][0]), int(want[1][1][0]), int(want[0][0][0]), int(want[1][0][0])]
    # through the wrapper the rows are fetched once more, and the pairs are the same
    _, _, rows, pairs = seg_lesion_match(ops, x, lab, "brats", None, 1, None)
    assert [len(r) for r in rows] == out["nrows"].tolist()
    assert all(np.array_equal(pairs[c].numpy(), want[c][2]) for c in range(2))


def test_argument_and_workspace_refusals_launch_nothing(ops):
    D, H, W = 5, 6, 7
    lib, stream = ops.lib, ops.stream
    cap, capp = 8, 8
    x = torch.zeros(3, D, H, W, device=DEV)
    lab = torch.zeros(D, H, W, dtype=torch.uint8, device=DEV)
    counts = torch.full((3, 4), 7, dtype=torch.int64, device=DEV)
    nrows = torch.full((6,), 7, dtype=torch.int64, device=DEV)
    rows = torch.full((6 * cap * 3,), 7, dtype=torch.int32, device=DEV)
    npairs = torch.full((3,), 7, dtype=torch.int64, device=DEV)
    pairs = torch.full((3 * capp * 3,), 7, dtype=torch.int32, device=DEV)
    need = lib.effq_seg_lesion_match_ws_bytes(3, D, H, W, cap, capp)
    assert need > lib.effq_cc_table_ws_bytes(6, D, H, W, cap)
    assert lib.effq_seg_lesion_match_ws_bytes(3, D, H, W, cap, 2 * capp) >= need
    for bad in ((0, D, H, W, cap, capp), (9, D, H, W, cap, capp), (3, 0, H, W, cap, capp), (3, D, H, W, 0, capp),
                (3, D, H, W, cap, 0), (3, D, H, W, cap, -1), (3, 2048, 1024, 1024, cap, capp),
                (3, D, H, W, cap, 2 ** 31 // 9 + 1)):
        assert lib.effq_seg_lesion_match_ws_bytes(*bad) == 0, bad
    assert lib.effq_seg_lesion_match_ws_bytes(3, D, H, W, cap, 2 ** 31 // 9) > 0       # 3 x 3 x that: just below 2^31 words
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    good = dict(x=_ptr(x), lab=_ptr(lab), C=3, dims=(D, H, W), mode=_lib.SEG_ARGMAX, fuse=0, conn=26, mr=cap, mp=capp,
                counts=_ptr(counts), nrows=_ptr(nrows), rows=_ptr(rows), npairs=_ptr(npairs), pairs=_ptr(pairs),
                ws=_ptr(ws), nbytes=need)

    def call(**over):
        a = dict(good, **over)
        return lib.effq_seg_lesion_match(a["x"], a["lab"], a["C"], *a["dims"], a["mode"], a["fuse"], 0.0, a["conn"],
                                         a["mr"], a["mp"], a["counts"], a["nrows"], a["rows"], a["npairs"], a["pairs"],
                                         a["ws"], a["nbytes"], stream)
    for over in (dict(conn=18), dict(mr=0), dict(mr=-5), dict(mp=0), dict(mp=-1), dict(mp=2 ** 31 // 9 + 1), dict(x=None),
                 dict(lab=None), dict(counts=None), dict(nrows=None), dict(rows=None), dict(npairs=None), dict(pairs=None),
                 dict(ws=None), dict(C=0), dict(C=9), dict(mode=2), dict(fuse=3), dict(dims=(2048, 1024, 1024)),
                 dict(dims=(D, 0, W))):
        assert call(**over) == ARG, over
    assert call(nbytes=need - 1) == WS
    assert call(nbytes=lib.effq_cc_table_ws_bytes(6, D, H, W, cap)) == WS        # the table's workspace is too short
    torch.cuda.synchronize()
    for t in (counts, nrows, rows, npairs, pairs):
        assert (t == 7).all()
    assert call() == 0                                                           # everything class 0
    torch.cuda.synchronize()
    assert counts.tolist() == [[1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]] and nrows.tolist() == [1, 0, 0, 1, 0, 0]
    assert npairs.tolist() == [1, 0, 0] and pairs[:3].tolist() == [0, 0, D * H * W] and (pairs[3:] == 7).all()
    with pytest.raises(_lib.EffqError):
        seg_lesion_match(ops, x, lab, "lits", None, None, 0)
    with pytest.raises(_lib.EffqError):
        seg_lesion_match(ops, x, lab, "lits", None, -1)
    with pytest.raises(_lib.EffqError):
        seg_lesion_match(ops, x, lab.float(), "lits")
    with pytest.raises(_lib.EffqError):
        seg_lesion_match(ops, x, lab, "lits", "agg")


# ---- the ptq mission with --lesion_match ----------------------------------------------------------------------------
def _run(tmp_path, name, task, fuse, match, data_dir, split_dir):
    from efficientq_amd import entrance
    snap = str(tmp_path / name)
    nmod, ncls = ("1", "3") if task == "lits" else ("4", "4")
    argv = ["ptq", "--task", task, "--qconv", "effq", "--qlvl_w", "4", "--qlvl_a", "4", "--q_first", "256,-1",
            "--q_last", "256,-1", "--width", "8,16,8", "--depth", "1,1,1", "--init_stride", "1", "--nMod", nmod,
            "--nClass", ncls, "--blk", "mid", "--ds", "simple", "--hetero_dim", "--drop_rate", "0.5",
            "--lwq_batchsz", "2", "--lwq_patchsz", "16,16,16", "--patch_size", "20,20,18", "--data_dir", data_dir,
            "--split_dir", split_dir, "--test_fp", "--save_nii", "--lesion_table", "--snap_dir", snap]
    if task == "brats":
        argv += ["--multi_label", "brats", "--merge_type", fuse]
    if match:
        argv.append("--lesion_match")
    entrance.main(argv)
    return snap


def _close(got, want):
    return abs(float(got) - want) <= 1e-7           # %.7g of a score in [0, 1] is within 5e-8 of it, the code within 1e-12


@pytest.mark.parametrize("task,fuse", [("lits", None), ("brats", "agg")])
def test_mission_writes_pairs_and_scores_that_the_maps_reproduce(tmp_path, task, fuse, capsys):
    shape = (20, 24, 18)
    val = ["c1", "c0"]
    data_dir, split_dir, arrays = write_dataset(str(tmp_path), task, ["c2", "c0", "c1"], shape, "npy",
                                                train=["c2", "c0"], val=val)
    snap = _run(tmp_path, "with", task, fuse, True, data_dir, split_dir)
    said = capsys.readouterr().out
    assert "[entrance] --lesion_match:" in said and "tp_l / fp_l / fn_l = " in said
    plain = _run(tmp_path, "without", task, fuse, False, data_dir, split_dir)
    assert "lesion_match" not in capsys.readouterr().out
    for folder in ("fp", "ptq"):
        with open(os.path.join(snap, folder, "metrics.csv"), "rb") as a, \
                open(os.path.join(plain, folder, "metrics.csv"), "rb") as b:
            assert a.read() == b.read()
        for name in ("lesion_match.csv", "lesion_pairs.csv"):
            assert not os.path.exists(os.path.join(plain, folder, name))
        # lesions.csv without its three new columns is the file of the run without the switch
        rows = list(csv.reader(open(os.path.join(snap, folder, "lesions.csv"))))
        assert rows[0][-3:] == ["match", "best_iou", "partners"]
        cut = "".join(",".join(r[:-3]) + "\r\n" for r in rows)
        assert cut.encode() == open(os.path.join(plain, folder, "lesions.csv"), "rb").read()
        order = list(dict.fromkeys(r[0] for r in csv.reader(open(os.path.join(snap, folder, "metrics.csv")))))[1:]
        assert sorted(order) == sorted(val)
        got_m = list(csv.reader(open(os.path.join(snap, folder, "lesion_match.csv"))))
        got_p = list(csv.reader(open(os.path.join(snap, folder, "lesion_pairs.csv"))))
        assert got_m[0] == ["subject", "class"] + list(LM.MATCH_COLUMNS)
        assert got_p[0] == ["subject", "class"] + list(LM.PAIR_COLUMNS)
        want_p, km, extra = [], 1, {}
        for sn in order:
            m, _ = read_nifti(os.path.join(snap, folder, "val", f"{sn}.nii.gz"))
            raw = arrays[sn][1]
            if task == "lits":
                pred = [m == c for c in range(3)]
                gt = [raw == c for c in range(3)]
            else:
                pred = [m > 0, (m == 1) | (m == 4), m == 4]
                gt = [raw > 0, (raw == 1) | (raw == 3), raw == 3]
            for c in range(3):
                a, b, pairs = ref_pairs(pred[c], gt[c])
                s = ref_scores(a, b, pairs)
                row = got_m[km]
                km += 1
                assert row[:5] == [sn, str(c), str(s["tp_l"]), str(s["fp_l"]), str(s["fn_l"])] and row[9] == str(s["groups"])
                assert all(_close(row[5 + k], s[name]) for k, name in enumerate(LM.SCORES)), (row, s)
                for i, j, n in pairs.tolist():
                    want_p.append([sn, str(c), str(i + 1), str(j + 1), str(n), n / (int(a[i]) + int(b[j]) - n)])
                for kind, side in (("label", s["label"]), ("pred", s["pred"])):
                    for k in range(len(side["match"])):
                        extra[(sn, str(c), kind, str(k + 1))] = (side["match"][k], side["best_iou"][k], side["partners"][k])
        assert km == len(got_m) and len(got_p) - 1 == len(want_p)
        for got, want in zip(got_p[1:], want_p):
            assert got[:5] == want[:5] and _close(got[5], want[5]), (got, want)
        assert len(rows) - 1 == len(extra)
        for r in rows[1:]:
            match, best, partners = extra[tuple(r[:4])]
            assert r[-3] == str(match) and _close(r[-2], best) and r[-1] == str(partners), r
