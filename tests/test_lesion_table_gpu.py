"""Per-lesion validation table on a real MI355X (-m gpu): effq_cc_table row for row against ref_table of
test_lesion_table_cpu (the masks of test_seg_lesions_gpu at both connectivities, several masks in one call, volumes whose
roots span several chunks of the rank scan), the truncation rule, effq_seg_lesion_table against the masks of the torch
restatements of test_seg_labels_gpu and against the tallies and the lesion counts, one full-size volume whose table is
known by construction, the argument checks, and the ptq mission with --lesion_table tied back to the maps it writes."""
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, evaluate as E
from efficientq_amd.hip_ops import get_ops
from efficientq_amd.nifti import read_nifti
from tests.test_lesion_table_cpu import ref_rows, ref_table
from tests.test_seg_eval_cpu import write_dataset
from tests.test_seg_labels_gpu import _logits, merge_basic, pred_lits
from tests.test_seg_lesions_gpu import CASES, _blocky, _checkerboard, _random

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = _lib.CC_TABLE_CHUNK


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _table_twice(ops, masks, conn, max_rows=None):
    """cc_table on a workspace filled with 0xFF, twice: the same bits both times."""
    m = torch.as_tensor(np.ascontiguousarray(masks), dtype=torch.uint8).to(DEV)
    ops.cc_table(m, conn, max_rows)                    # sizes the workspace
    ops._ws["cc"].fill_(0xFF)
    rows1, n1 = ops.cc_table(m, conn, max_rows)
    ops._ws["cc"].fill_(0xFF)
    rows2, n2 = ops.cc_table(m, conn, max_rows)
    if m.dim() == 3:
        rows1, rows2, n1, n2 = [rows1], [rows2], n1.reshape(1), n2.reshape(1)
    assert n1.dtype == torch.int64 and torch.equal(n1, n2)
    for a, b in zip(rows1, rows2):
        assert a.dtype == torch.int32 and a.dim() == 2 and a.shape[1] == 2 and torch.equal(a, b)
    return [r.numpy().astype(np.int64) for r in rows1], n1.numpy()


def _check(ops, mask, conn, max_rows=None):
    got, n = _table_twice(ops, mask, conn, max_rows)
    want = ref_rows(mask, None, conn)[:, :2]
    assert int(n[0]) == len(want)
    assert got[0].shape == want.shape and np.array_equal(got[0], want), \
        f"{int((got[0] != want).any(1).sum())} of {len(want)} rows differ"
    return want


# ---- cc_table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [26, 6])
@pytest.mark.parametrize("case", sorted(CASES))
def test_cc_table_equals_the_reference_table(ops, case, conn):
    mask = CASES[case]()
    want = _check(ops, mask, conn)
    if case == "empty":
        assert len(want) == 0
    if case == "full":
        assert want.tolist() == [[0, mask.size]]
    if case == "checkerboard" and conn == 6:
        assert len(want) == int(mask.sum()) and (want[:, 1] == 1).all()
    if case == "serpentine":
        assert want.tolist() == [[0, int(mask.sum())]]


@pytest.mark.parametrize("conn", [26, 6])
def test_four_masks_in_one_call_do_not_leak(ops, conn):
    shape = (13, 18, 41)
    masks = np.stack([_random(shape, 0.3, 11), np.zeros(shape, np.uint8), np.ones(shape, np.uint8),
                      _random(shape, 0.05, 12)])
    got, n = _table_twice(ops, masks, conn)
    for p in range(4):
        want = ref_rows(masks[p], None, conn)[:, :2]
        assert int(n[p]) == len(want), p
        assert np.array_equal(got[p], want), p


@pytest.mark.parametrize("shape", [(8, 16, 64), (7, 19, 53), (3, 5, CHUNK + 1)])
def test_roots_in_several_chunks_of_the_scan(ops, shape):
    """8192 voxels = 4 whole chunks; 7049 and 3 x 5 x 2049: a last chunk that is cut short, with roots in it."""
    mask = _random(shape, 0.08, 21)
    mask[-2:, -2:, -2:] = 0
    mask[-1, -1, -1] = 1                                # the last voxel is a component of its own
    for conn in (26, 6):
        want = _check(ops, mask, conn)
        assert len(set((want[:, 0] // CHUNK).tolist())) >= 3
        assert want[-1].tolist() == [mask.size - 1, 1]
    assert (mask.size % CHUNK == 0) == (shape == (8, 16, 64))


# ---- truncation -----------------------------------------------------------------------------------------------------
def test_a_short_table_holds_the_first_rows_and_nothing_is_written_past_it(ops):
    mask = _checkerboard((12, 13, 37))                  # at 6 every foreground voxel is a component of its own
    want = ref_rows(mask, None, 6)[:, :2]
    total = int(mask.sum())
    assert len(want) == total and total > 2000
    m = torch.from_numpy(mask).to(DEV)
    D, H, W = mask.shape
    for cap in (1000, total):
        need = ops.lib.effq_cc_table_ws_bytes(1, D, H, W, cap)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        guard = 4096
        rows = torch.full((cap * 2 + guard,), -7, dtype=torch.int32, device=DEV)
        nrows = torch.full((2,), -7, dtype=torch.int64, device=DEV)
        rc = ops.lib.effq_cc_table(_ptr(m), 1, D, H, W, 6, cap, _ptr(rows), _ptr(nrows), _ptr(ws), need, ops.stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert nrows.tolist() == [total, -7]
        assert np.array_equal(rows[:cap * 2].view(cap, 2).cpu().numpy(), want[:cap])
        assert (rows[cap * 2:] == -7).all()
    # through HipOps a table that was too short is fetched once more, whole
    for cap in (1000, total, total + 1, None):
        got, n = ops.cc_table(m, 6, cap)
        assert int(n) == total and np.array_equal(got.numpy(), want), cap


# ---- seg_lesion_table -----------------------------------------------------------------------------------------------
SHAPE = (12, 20, 40)
RAGGED = (7, 9, 11)                                     # 693 voxels: the scalar path of the masks


def _check_case(ops, x, lab, task, fuse, pred, gt):
    Cc = x.shape[0]
    ops.seg_lesion_table(x, lab, task, fuse)
    ops._ws["cc"].fill_(0xFF)
    counts, nrows, rows = ops.seg_lesion_table(x, lab, task, fuse)
    ops._ws["cc"].fill_(0xFF)
    counts2, nrows2, rows2 = ops.seg_lesion_table(x, lab, task, fuse)
    assert torch.equal(counts, counts2) and torch.equal(nrows, nrows2)
    assert all(torch.equal(a, b) for a, b in zip(rows, rows2))
    assert counts.dtype == torch.int64 and counts.shape == (Cc, 4) and nrows.shape == (2 * Cc,) and len(rows) == 2 * Cc
    assert torch.equal(counts, ops.seg_lesions(x, lab, task, fuse).cpu())
    tal = ops.seg_tallies(x, lab, task, fuse).tolist()
    for c in range(Cc):
        want_p, want_l = ref_table(pred[c], gt[c])
        got_p, got_l = rows[c].numpy().astype(np.int64), rows[Cc + c].numpy().astype(np.int64)
        assert np.array_equal(got_p, want_p), (c, "pred")
        assert np.array_equal(got_l, want_l), (c, "label")
        tp, fp, fn, tn = tal[c]
        totall, predl, fnl, fpl = counts[c].tolist()
        assert int(nrows[c]) == predl == len(got_p) and int(nrows[Cc + c]) == totall == len(got_l)
        assert got_p[:, 1].sum() == tp + fp and got_l[:, 1].sum() == tp + fn
        assert got_p[:, 2].sum() == tp and got_l[:, 2].sum() == tp
        assert int((got_p[:, 2] == 0).sum()) == fpl and int((got_l[:, 2] == 0).sum()) == fnl


@pytest.mark.parametrize("C", [2, 3])
def test_argmax_table_equals_the_restatement(ops, C):
    x = _logits(ops, 1, C, SHAPE, 30 + C, sigmoid=False)[0]
    lab = _blocky(SHAPE, C, 40 + C).to(DEV)
    pred = pred_lits(x[None])[0].cpu().numpy()
    labn = lab.cpu().numpy()
    _check_case(ops, x, lab, "lits", None, [pred == c for c in range(C)], [labn == c for c in range(C)])


@pytest.mark.parametrize("fuse", [None, "agg", "con"])
def test_sigmoid_table_equals_the_restatement(ops, fuse):
    x = _logits(ops, 1, 3, SHAPE, 53, sigmoid=True)[0]
    lab = _blocky(SHAPE, 2, 63, channels=3).to(DEV)
    hard = merge_basic((torch.sigmoid(x[None]) >= 0.5).int(), fuse)[0].cpu().numpy()
    _check_case(ops, x, lab, "brats", fuse, hard, lab.cpu().numpy())


@pytest.mark.parametrize("task", ["lits", "brats"])
def test_ragged_volume_takes_the_scalar_mask_path(ops, task):
    assert (RAGGED[0] * RAGGED[1] * RAGGED[2]) % 4 != 0
    cut = (slice(0, RAGGED[0]), slice(0, RAGGED[1]), slice(0, RAGGED[2]))
    if task == "lits":
        x = _logits(ops, 1, 3, RAGGED, 71, sigmoid=False)[0]
        lab = _blocky((8, 12, 12), 3, 72)[cut].contiguous().to(DEV)
        pred, labn = pred_lits(x[None])[0].cpu().numpy(), lab.cpu().numpy()
        _check_case(ops, x, lab, "lits", None, [pred == c for c in range(3)], [labn == c for c in range(3)])
    else:
        x = _logits(ops, 1, 3, RAGGED, 73, sigmoid=True)[0]
        lab = _blocky((8, 12, 12), 2, 74, channels=3)[(slice(None),) + cut].contiguous().to(DEV)
        hard = merge_basic((torch.sigmoid(x[None]) >= 0.5).int(), "agg")[0].cpu().numpy()
        _check_case(ops, x, lab, "brats", "agg", hard, lab.cpu().numpy())


def test_full_size_volume_known_by_construction(ops):
    """155 x 240 x 240, built on the device: one labelled box in each cell of 24^3 of a 6 x 10 x 10 grid, of extents
    e0 x e1 x e2 from the cell's number, and the same box predicted two voxels further along w.  Class 1 is the boxes:
    row k of both planes is cell k, size e0 e1 e2, overlap e0 e1 max(e2 - 2, 0) - boxes no wider than 2 are missed and
    invented.  Class 0 is everything else: one component from voxel 0 in each plane, the giant one."""
    D, H, W = 155, 240, 240
    S = D * H * W
    lab = torch.zeros(D, H, W, dtype=torch.uint8, device=DEV)
    pred = torch.zeros(D, H, W, dtype=torch.uint8, device=DEV)
    want_l, want_p = [], []
    for k in range(600):
        cd, ch, cw = k // 100, (k // 10) % 10, k % 10
        z, y, x = 24 * cd + 2, 24 * ch + 2, 24 * cw + 2
        e0, e1, e2 = 1 + k % 7, 1 + (k // 7) % 8, 1 + (5 * k) % 8
        lab[z:z + e0, y:y + e1, x:x + e2] = 1
        pred[z:z + e0, y:y + e1, x + 2:x + 2 + e2] = 1
        ov = e0 * e1 * max(e2 - 2, 0)
        want_l.append([(z * H + y) * W + x, e0 * e1 * e2, ov])
        want_p.append([(z * H + y) * W + x + 2, e0 * e1 * e2, ov])
    want_l, want_p = np.array(want_l, np.int64), np.array(want_p, np.int64)
    assert (np.diff(want_l[:, 0]) > 0).all() and (want_l[:, 2] == 0).sum() > 100
    logits = torch.stack([torch.full((D, H, W), 0.5, device=DEV), pred.float()])
    counts, nrows, rows = ops.seg_lesion_table(logits, lab, "lits")
    missed = int((want_l[:, 2] == 0).sum())
    assert counts.tolist() == [[1, 1, 0, 0], [600, 600, missed, missed]]
    assert nrows.tolist() == [1, 600, 1, 600]
    assert np.array_equal(rows[1].numpy(), want_p) and np.array_equal(rows[3].numpy(), want_l)
    vol, union = int(want_l[:, 1].sum()), int(2 * want_l[:, 1].sum() - want_l[:, 2].sum())
    assert rows[0].tolist() == [[0, S - vol, S - union]] and rows[2].tolist() == [[0, S - vol, S - union]]
    assert torch.equal(counts, ops.seg_lesions(logits, lab, "lits").cpu())
    # the predicted plane alone, as a mask: the same firsts and sizes
    got, n = ops.cc_table(pred, 26)
    assert int(n) == 600 and np.array_equal(got.numpy(), want_p[:, :2])


# ---- argument checks ------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(ops):
    D, H, W = 5, 6, 7
    lib, stream = ops.lib, ops.stream
    m = torch.ones(D, H, W, dtype=torch.uint8, device=DEV)
    cap = 8
    rows = torch.full((cap * 3 * 6,), 7, dtype=torch.int32, device=DEV)
    nrows = torch.full((6,), 7, dtype=torch.int64, device=DEV)
    counts = torch.full((3, 4), 7, dtype=torch.int64, device=DEV)
    need = lib.effq_cc_table_ws_bytes(1, D, H, W, cap)
    assert need > lib.effq_cc_ws_bytes(1, D, H, W) > 0
    assert lib.effq_cc_table_ws_bytes(1, D, H, W, 0) == 0 and lib.effq_cc_table_ws_bytes(1, 0, H, W, cap) == 0
    assert lib.effq_cc_table_ws_bytes(1, 2048, 1024, 1024, cap) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    ARG, WS = 1, 3
    call = lambda mask, conn, mr, r, n, w, nbytes, dims=(1, D, H, W): lib.effq_cc_table(
        mask, *dims, conn, mr, r, n, w, nbytes, stream)
    assert call(_ptr(m), 18, cap, _ptr(rows), _ptr(nrows), _ptr(ws), need) == ARG
    assert call(_ptr(m), 26, 0, _ptr(rows), _ptr(nrows), _ptr(ws), need) == ARG
    assert call(_ptr(m), 26, -1, _ptr(rows), _ptr(nrows), _ptr(ws), need) == ARG
    assert call(None, 26, cap, _ptr(rows), _ptr(nrows), _ptr(ws), need) == ARG
    assert call(_ptr(m), 26, cap, None, _ptr(nrows), _ptr(ws), need) == ARG
    assert call(_ptr(m), 26, cap, _ptr(rows), None, _ptr(ws), need) == ARG
    assert call(_ptr(m), 26, cap, _ptr(rows), _ptr(nrows), None, need) == ARG
    assert call(_ptr(m), 26, cap, _ptr(rows), _ptr(nrows), _ptr(ws), need, (1, 2048, 1024, 1024)) == ARG
    assert call(_ptr(m), 26, cap, _ptr(rows), _ptr(nrows), _ptr(ws), need, (0, D, H, W)) == ARG
    assert call(_ptr(m), 6, cap, _ptr(rows), _ptr(nrows), _ptr(ws), need - 1) == WS
    with pytest.raises(_lib.EffqError):
        _lib.check(WS, "effq_cc_table")

    x = torch.zeros(3, D, H, W, device=DEV)
    lab = torch.zeros(D, H, W, dtype=torch.uint8, device=DEV)
    need3 = lib.effq_cc_table_ws_bytes(6, D, H, W, cap)
    ws3 = torch.zeros(need3, dtype=torch.uint8, device=DEV)
    good = dict(x=_ptr(x), lab=_ptr(lab), C=3, dims=(D, H, W), mode=_lib.SEG_ARGMAX, fuse=0, conn=26, mr=cap,
                counts=_ptr(counts), nrows=_ptr(nrows), rows=_ptr(rows), ws=_ptr(ws3), nbytes=need3)

    def seg(**over):
        a = dict(good, **over)
        return lib.effq_seg_lesion_table(a["x"], a["lab"], a["C"], *a["dims"], a["mode"], a["fuse"], 0.0, a["conn"],
                                         a["mr"], a["counts"], a["nrows"], a["rows"], a["ws"], a["nbytes"], stream)
    for over in (dict(conn=18), dict(mr=0), dict(mr=-5), dict(x=None), dict(lab=None), dict(counts=None),
                 dict(nrows=None), dict(rows=None), dict(ws=None), dict(C=0), dict(C=9), dict(mode=2), dict(fuse=3),
                 dict(dims=(2048, 1024, 1024)), dict(dims=(D, 0, W))):
        assert seg(**over) == ARG, over
    assert seg(nbytes=need3 - 1) == WS
    torch.cuda.synchronize()
    assert (rows == 7).all() and (nrows == 7).all() and (counts == 7).all()
    assert seg() == 0                                                            # everything class 0
    torch.cuda.synchronize()
    assert counts.tolist() == [[1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]] and nrows.tolist() == [1, 0, 0, 1, 0, 0]
    assert rows[:3].tolist() == [0, D * H * W, D * H * W] and rows[3 * cap * 3:3 * cap * 3 + 3].tolist() == rows[:3].tolist()
    with pytest.raises(_lib.EffqError):
        ops.cc_table(m, 18)
    with pytest.raises(_lib.EffqError):
        ops.cc_table(m, 26, 0)
    with pytest.raises(_lib.EffqError):
        ops.cc_table(m.float())
    with pytest.raises(_lib.EffqError):
        ops.seg_lesion_table(x, lab, "lits", None, -1)
    with pytest.raises(_lib.EffqError):
        ops.seg_lesion_table(x, lab.float(), "lits")
    with pytest.raises(_lib.EffqError):
        ops.seg_lesion_table(x, lab, "lits", "agg")


# ---- validate_seg and the ptq mission with --lesion_table -----------------------------------------------------------
def _run(tmp_path, name, task, fuse, table, data_dir, split_dir):
    from efficientq_amd import entrance
    snap = str(tmp_path / name)
    nmod, ncls = ("1", "3") if task == "lits" else ("4", "4")
    argv = ["ptq", "--task", task, "--qconv", "effq", "--qlvl_w", "4", "--qlvl_a", "4", "--q_first", "256,-1",
            "--q_last", "256,-1", "--width", "8,16,8", "--depth", "1,1,1", "--init_stride", "1", "--nMod", nmod,
            "--nClass", ncls, "--blk", "mid", "--ds", "simple", "--hetero_dim", "--drop_rate", "0.5",
            "--lwq_batchsz", "2", "--lwq_patchsz", "16,16,16", "--patch_size", "20,20,18", "--data_dir", data_dir,
            "--split_dir", split_dir, "--test_fp", "--save_nii", "--is_cc", "--snap_dir", snap]
    if task == "brats":
        argv += ["--multi_label", "brats", "--merge_type", fuse]
    if table:
        argv.append("--lesion_table")
    entrance.main(argv)
    return snap


@pytest.mark.parametrize("task,fuse", [("lits", None), ("brats", "agg")])
def test_mission_writes_a_lesions_csv_that_the_maps_reproduce(tmp_path, task, fuse, capsys):
    shape = (20, 24, 18)
    val = ["c1", "c0"]
    data_dir, split_dir, arrays = write_dataset(str(tmp_path), task, ["c2", "c0", "c1"], shape, "npy",
                                                train=["c2", "c0"], val=val)
    snap = _run(tmp_path, "with", task, fuse, True, data_dir, split_dir)
    assert "label lesions detected / all, by size in voxels" in capsys.readouterr().out
    plain = _run(tmp_path, "without", task, fuse, False, data_dir, split_dir)
    for folder in ("fp", "ptq"):
        with open(os.path.join(snap, folder, "metrics.csv"), "rb") as a, \
                open(os.path.join(plain, folder, "metrics.csv"), "rb") as b:
            assert a.read() == b.read()
        assert not os.path.exists(os.path.join(plain, folder, "lesions.csv"))
        got = list(csv.reader(open(os.path.join(snap, folder, "lesions.csv"))))
        assert got[0] == ["subject", "class", "kind", "lesion", "d", "h", "w", "size", "overlap"]
        order = list(dict.fromkeys(r[0] for r in csv.reader(open(os.path.join(snap, folder, "metrics.csv")))))[1:]
        assert sorted(order) == sorted(val)             # the subjects in the order of metrics.csv
        want = []
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
                pr, lr = ref_table(pred[c], gt[c])
                for kind, rows in (("label", lr), ("pred", pr)):
                    for k, (first, size, ov) in enumerate(rows.tolist()):
                        d, h, w = np.unravel_index(first, shape)
                        want.append([sn, str(c), kind, str(k + 1), str(d), str(h), str(w), str(size), str(ov)])
        assert got[1:] == want, folder


def test_validate_seg_keys_and_the_shared_call(ops):
    """lesion_table=False: the keys of before; with it one more key (two with a spacing), and with lesions=True the same
    counts as the call of their own."""
    from efficientq_amd import calibrate as K, config as Cf, synth
    args = Cf.make_args(Cf.TINY_NET, 4, 4)
    QConv, _, kwQ = Cf.get_conv_class(args)
    model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
    synth.randomise_network(model, 0)
    model.eval()
    K.search_fold_and_remove_bn(model)
    model.to(DEV)
    K.set_fp(model)
    g = torch.Generator().manual_seed(1)
    shape = (20, 24, 18)
    loader = [(torch.randn(1, 1, *shape, generator=g), torch.randint(0, 3, (1,) + shape, generator=g))]
    plain = E.validate_seg(model, loader, "lits", (16, 16, 16), 4)
    cc = E.validate_seg(model, loader, "lits", (16, 16, 16), 4, lesions=True)
    tab = E.validate_seg(model, loader, "lits", (16, 16, 16), 4, lesion_table=True)
    both = E.validate_seg(model, loader, "lits", (16, 16, 16), 4, lesions=True, lesion_table=True,
                          geometry=(2.0, 1.0, 0.5))
    assert set(plain[0]) == {"name", "counts", "dsc", "sens", "spec", "acc"}
    assert set(tab[0]) == set(plain[0]) | {"lesion_table"}
    assert set(both[0]) == set(plain[0]) | {"lesion_table", "lesions", "spacing"}
    assert torch.equal(both[0]["lesions"], cc[0]["lesions"]) and both[0]["spacing"] == (2.0, 1.0, 0.5)
    assert len(tab[0]["lesion_table"]) == 3
    for c, (lab_rows, pred_rows) in enumerate(tab[0]["lesion_table"]):
        totall, predl, fnl, fpl = cc[0]["lesions"][c].tolist()
        tp, fp, fn, tn = plain[0]["counts"][c].tolist()
        assert lab_rows.dtype == np.int64 and lab_rows.shape == (totall, 5) and pred_rows.shape == (predl, 5)
        assert lab_rows[:, 3].sum() == tp + fn and pred_rows[:, 3].sum() == tp + fp
        assert int((lab_rows[:, 4] == 0).sum()) == fnl and int((pred_rows[:, 4] == 0).sum()) == fpl
        want = ref_rows(loader[0][1][0].numpy() == c)
        assert np.array_equal(np.ravel_multi_index(tuple(lab_rows[:, :3].T), shape), want[:, 0])
        assert np.array_equal(lab_rows[:, 3], want[:, 1])
        assert np.array_equal(both[0]["lesion_table"][c][0], lab_rows)
