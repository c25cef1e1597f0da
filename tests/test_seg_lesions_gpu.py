"""Connected components and the lesion-level metrics on a real MI355X (-m gpu): effq_cc_label voxel for voxel against
the numpy labeller of test_seg_lesions_cpu (both connectivities, ragged and degenerate extents, long paths, contacts
through tile corners and edges, several masks in one call), one full-size volume whose answer is known by construction,
effq_seg_lesions against the restatement of metrics.py:69-94 on the masks of the torch restatements of
test_seg_labels_gpu, its argument checks, and the ptq mission with --is_cc tied back to the label maps it writes."""
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, evaluate as E
from efficientq_amd.hip_ops import get_ops
from efficientq_amd.nifti import read_nifti
from tests.test_seg_eval_cpu import write_dataset
from tests.test_seg_labels_gpu import _logits, merge_basic, pred_lits
from tests.test_seg_lesions_cpu import lesion_counts, num_components, ref_label

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def _label_twice(ops, masks, conn):
    """cc_label on a workspace filled with 0xFF, twice: the same bits both times."""
    m = torch.as_tensor(np.ascontiguousarray(masks), dtype=torch.uint8).to(DEV)
    ops.cc_label(m, conn)                    # sizes the workspace
    ops._ws["cc"].fill_(0xFF)
    lab1, n1 = ops.cc_label(m, conn)
    lab1, n1 = lab1.clone(), n1.clone()
    ops._ws["cc"].fill_(0xFF)
    lab2, n2 = ops.cc_label(m, conn)
    assert lab1.dtype == torch.int32 and lab1.shape == m.shape and n1.dtype == torch.int64
    assert torch.equal(lab1, lab2) and torch.equal(n1, n2)
    return lab1.cpu().numpy(), n1.cpu().numpy()


def _check(ops, mask, conn):
    got, n = _label_twice(ops, mask, conn)
    want = ref_label(mask, conn)
    assert np.array_equal(got, want), f"{int((got != want).sum())} voxels differ"
    assert int(n) == num_components(want) == num_components(got)
    return want


# ---- masks ----------------------------------------------------------------------------------------------------------
def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _checkerboard(shape):
    d, h, w = np.indices(shape)
    return ((d + h + w) % 2 == 0).astype(np.uint8)


def _serpentine(D=11, H=18, W=70):
    """A one-voxel-wide path: up through the even planes on w < W/2, over a bridge in the last plane, and down again on
    w > W/2.  It crosses every tile border many times and ends two voxels from where it started."""
    M = W // 2
    m = np.zeros((D, H, W), np.uint8)
    for lo, hi, inner in ((0, M - 1, M - 1), (M + 1, W - 1, M + 1)):
        w = inner                                     # the cursor: both halves start at h = 0 next to the middle
        other = {lo: hi, hi: lo}
        planes = list(range(0, D, 2))
        for k, d in enumerate(planes):
            rows = list(range(0, H, 2))
            if k % 2:
                rows.reverse()
            for j, h in enumerate(rows):
                m[d, h, lo:hi + 1] = 1
                w = other[w]                          # the row is walked to its other end
                if j + 1 < len(rows):
                    m[d, (h + rows[j + 1]) // 2, w] = 1
            if k + 1 < len(planes):
                m[d + 1, rows[-1], w] = 1
        last_row = rows[-1]
    m[planes[-1], last_row, M] = 1                    # the bridge
    assert m[0, 0, M - 1] and m[0, 0, M + 1] and not m[0, :2, M].any()
    return m


def _corner_and_edge_contacts():
    """Components that meet only through a tile corner or a tile edge (tiles of 8 x 8 x 32)."""
    m = np.zeros((16, 16, 64), np.uint8)
    m[6:8, 6:8, 30:32] = 1
    m[8:10, 8:10, 32:34] = 1          # (7, 7, 31) - (8, 8, 32): through the corner of four... eight tiles
    m[7, 7, 3:6] = 1
    m[8, 8, 3:6] = 1                  # along w: through the d / h edge
    m[3, 7, 31] = 1
    m[3, 8, 32] = 1                   # through the h / w edge
    m[7, 12, 63] = 1
    m[8, 12, 62] = 1                  # a d face, diagonal in w
    m[15, 15, 40:50] = 1
    m[14, 14, 50:60] = 1
    return m


def _first_and_last():
    m = _random((19, 21, 45), 0.04, 5)
    m[0, 0, :] = 1
    m[0, :, -1] = 1
    m[:, -1, -1] = 1
    return m


CASES = {
    "ragged": lambda: _random((37, 50, 29), 0.3, 1),
    "line_w": lambda: _random((1, 1, 300), 0.6, 2),
    "line_d": lambda: _random((64, 1, 1), 0.6, 3),
    "sheet": lambda: _random((1, 40, 40), 0.3, 4),
    "empty": lambda: np.zeros((17, 20, 70), np.uint8),
    "full": lambda: np.ones((17, 20, 70), np.uint8),
    "checkerboard": lambda: _checkerboard((12, 13, 37)),
    "dust": lambda: _random((30, 40, 66), 0.05, 6),
    "sparse": lambda: _random((30, 40, 66), 0.3, 7),
    "dense": lambda: _random((30, 40, 66), 0.6, 8),
    "contacts": _corner_and_edge_contacts,
    "serpentine": _serpentine,
    "first_and_last": _first_and_last,
}


@pytest.mark.parametrize("conn", [26, 6])
@pytest.mark.parametrize("case", sorted(CASES))
def test_cc_label_equals_the_reference_labeller(ops, case, conn):
    mask = CASES[case]()
    want = _check(ops, mask, conn)
    n = num_components(want)
    if case == "empty":
        assert n == 0
    if case == "full":
        assert n == 1 and (want == 1).all()
    if case == "checkerboard":
        assert n == (1 if conn == 26 else int(mask.sum()))
    if case == "serpentine":
        assert n == 1 and np.array_equal(want, mask.astype(np.int32))      # the path holds voxel 0
    if case == "first_and_last":
        assert want[0, 0, 0] == 1 and want[-1, -1, -1] == 1
    if case == "contacts":
        assert n == (5 if conn == 26 else 10)


@pytest.mark.parametrize("conn", [26, 6])
def test_six_masks_in_one_call_do_not_leak(ops, conn):
    shape = (13, 18, 41)
    masks = np.stack([_random(shape, 0.3, 11), np.zeros(shape, np.uint8), np.ones(shape, np.uint8),
                      _checkerboard(shape), _random(shape, 0.05, 12), _random(shape, 0.6, 13)])
    got, n = _label_twice(ops, masks, conn)
    for p in range(6):
        want = ref_label(masks[p], conn)
        assert np.array_equal(got[p], want), p
        assert int(n[p]) == num_components(want)


def test_full_size_volume_known_by_construction(ops):
    """155 x 240 x 240: one blob in each cell of 24^3 of a 6 x 10 x 10 grid (boxes, and balls in every third cell), well
    apart from one another; in every fourth cell a second box starts at the corner diagonally behind the first box's
    last voxel - one component at 26, two at 6.  No labeller is run: the label of a blob is 1 + its first voxel."""
    D, H, W = 155, 240, 240
    mask = np.zeros((D, H, W), np.uint8)
    want26, want6 = np.zeros((D, H, W), np.int32), np.zeros((D, H, W), np.int32)
    lin = lambda d, h, w: (d * H + h) * W + w
    rng = np.random.default_rng(0)
    blobs = pairs = 0
    for cd in range(6):
        for ch in range(10):
            for cw in range(10):
                k = (cd * 10 + ch) * 10 + cw
                z, y, x = 24 * cd + 2, 24 * ch + 2, 24 * cw + 2          # the blob lives in [2, 22) of its cell
                if k % 3 == 0:
                    r = int(rng.integers(2, 9))
                    c = np.array([z + 9, y + 9, x + 9])
                    g = np.indices((20, 20, 20)) + np.array([z, y, x])[:, None, None, None]
                    ball = ((g - c[:, None, None, None]) ** 2).sum(0) <= r * r
                    sl = (slice(z, z + 20), slice(y, y + 20), slice(x, x + 20))
                    first = 1 + lin(c[0] - r, c[1], c[2])
                    mask[sl][ball] = 1
                    want26[sl][ball] = first
                    want6[sl][ball] = first
                else:
                    e = rng.integers(1, 9, 3)
                    sl = (slice(z, z + e[0]), slice(y, y + e[1]), slice(x, x + e[2]))
                    mask[sl] = 1
                    want26[sl] = want6[sl] = 1 + lin(z, y, x)
                    if k % 4 == 0:
                        z2, y2, x2 = z + e[0], y + e[1], x + e[2]
                        f = rng.integers(1, 9, 3)
                        sl2 = (slice(z2, z2 + f[0]), slice(y2, y2 + f[1]), slice(x2, x2 + f[2]))
                        mask[sl2] = 1
                        want26[sl2] = 1 + lin(z, y, x)
                        want6[sl2] = 1 + lin(z2, y2, x2)
                        pairs += 1
                blobs += 1
    assert blobs == 600 and pairs > 50
    m = torch.from_numpy(mask).to(DEV)
    for conn, want, n in ((26, want26, blobs), (6, want6, blobs + pairs)):
        lab, ncomp = ops.cc_label(m, conn)
        assert int(ncomp) == n
        assert torch.equal(lab, torch.from_numpy(want).to(DEV))


# ---- seg_lesions ----------------------------------------------------------------------------------------------------
SHAPE = (12, 20, 40)


def _blocky(shape, nvals, seed, channels=None):
    """Labels made of 2 x 4 x 4 blocks of one value, so that the components are more than dust."""
    g = torch.Generator().manual_seed(seed)
    lead = () if channels is None else (channels,)
    small = torch.randint(0, nvals, lead + (shape[0] // 2, shape[1] // 4, shape[2] // 4), generator=g)
    return small.repeat_interleave(2, -3).repeat_interleave(4, -2).repeat_interleave(4, -1).to(torch.uint8)


def _check_lesions(ops, x, lab, task, fuse, pred, gt):
    got = ops.seg_lesions(x, lab, task, fuse)
    assert got.dtype == torch.int64 and got.shape == (x.shape[0], 4)
    again = ops.seg_lesions(x, lab, task, fuse)
    assert torch.equal(got, again)
    want = [lesion_counts(pred[c], gt[c]) for c in range(x.shape[0])]
    print(task, fuse, "lesions", got.tolist())
    assert got.tolist() == want
    tal = ops.seg_tallies(x, lab, task, fuse).tolist()
    for c, ((tp, fp, fn, tn), (totall, predl, fnl, fpl)) in enumerate(zip(tal, got.tolist())):
        if tp == 0:
            assert fnl == totall and fpl == predl, c
        if tp + fn == 0:
            assert totall == 0, c
        assert fnl <= totall and fpl <= predl


@pytest.mark.parametrize("C", [2, 3, 8])
def test_argmax_lesions_equal_the_restatement(ops, C):
    x = _logits(ops, 1, C, SHAPE, 30 + C, sigmoid=False)[0]            # ties and NaNs
    lab = _blocky(SHAPE, C, 40 + C).to(DEV)
    pred = pred_lits(x[None])[0].cpu().numpy()
    labn = lab.cpu().numpy()
    _check_lesions(ops, x, lab, "lits", None, [pred == c for c in range(C)], [labn == c for c in range(C)])


@pytest.mark.parametrize("fuse", [None, "agg", "con"])
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_sigmoid_lesions_equal_the_restatement(ops, C, fuse):
    x = _logits(ops, 1, C, SHAPE, 50 + C, sigmoid=True)[0]             # the threshold and 1024 ulps either side of it
    lab = _blocky(SHAPE, 2, 60 + C, channels=C).to(DEV)
    hard = merge_basic((torch.sigmoid(x[None]) >= 0.5).int(), fuse)[0].cpu().numpy()
    _check_lesions(ops, x, lab, "brats", fuse, hard, lab.cpu().numpy())


def test_smooth_logits_give_few_large_lesions(ops):
    """Blocky logits as well: components that span tiles on both sides, and an unaligned logits pointer."""
    g = torch.Generator().manual_seed(3)
    shape = (18, 28, 68)
    small = torch.randn(3, 6, 7, 17, generator=g)
    x = small.repeat_interleave(3, 1).repeat_interleave(4, 2).repeat_interleave(4, 3).contiguous()
    lab = _blocky(shape, 2, 4, channels=3)[:, :18].contiguous().to(DEV)
    buf = torch.empty(1 + x.numel(), device=DEV)
    y = buf[1:].view(x.shape)
    y.copy_(x)
    assert y.data_ptr() % 16 != 0
    hard = merge_basic((torch.sigmoid(y[None]) >= 0.5).int(), "agg")[0].cpu().numpy()
    _check_lesions(ops, y, lab, "brats", "agg", hard, lab.cpu().numpy())


# ---- argument checks ------------------------------------------------------------------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_argument_errors_leave_the_outputs_untouched(ops):
    D, H, W = 5, 6, 7
    m = torch.ones(D, H, W, dtype=torch.uint8, device=DEV)
    labels = torch.full((D, H, W), 7, dtype=torch.int32, device=DEV)
    ncomp = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    need = ops.lib.effq_cc_ws_bytes(1, D, H, W)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    stream = ops.stream
    for conn, nbytes in ((18, need), (26, need - 1), (6, 0)):
        rc = ops.lib.effq_cc_label(_ptr(m), 1, D, H, W, conn, _ptr(labels), _ptr(ncomp), _ptr(ws), nbytes, stream)
        assert rc != 0
        with pytest.raises(_lib.EffqError):
            _lib.check(rc, "effq_cc_label")
    assert ops.lib.effq_cc_label(None, 1, D, H, W, 26, _ptr(labels), _ptr(ncomp), _ptr(ws), need, stream) != 0
    assert ops.lib.effq_cc_ws_bytes(1, 2048, 1024, 1024) == 0 and ops.lib.effq_cc_ws_bytes(1, 0, 4, 4) == 0
    x = torch.zeros(3, D, H, W, device=DEV)
    lab = torch.zeros(D, H, W, dtype=torch.uint8, device=DEV)
    counts = torch.full((3, 4), 7, dtype=torch.int64, device=DEV)
    need3 = ops.lib.effq_cc_ws_bytes(6, D, H, W)
    ws3 = torch.zeros(need3, dtype=torch.uint8, device=DEV)
    for conn, nbytes in ((18, need3), (26, need3 - 1)):
        rc = ops.lib.effq_seg_lesions(_ptr(x), _ptr(lab), 3, D, H, W, _lib.SEG_ARGMAX, 0, 0.0, conn, _ptr(counts),
                                      _ptr(ws3), nbytes, stream)
        assert rc != 0
    rc = ops.lib.effq_seg_lesions(_ptr(x), _ptr(lab), 3, D, H, W, _lib.SEG_ARGMAX, 0, 0.0, 26, _ptr(counts), _ptr(ws3),
                                  need3, stream)
    assert rc == 0 and counts.tolist() == [[1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]      # everything class 0
    counts.fill_(7)
    torch.cuda.synchronize()
    with pytest.raises(_lib.EffqError):
        ops.cc_label(m, 18)
    with pytest.raises(_lib.EffqError):
        ops.cc_label(m.float())
    with pytest.raises(_lib.EffqError):
        ops.cc_label(m.cpu())
    for bad_lab, task, fuse in ((lab.float(), "lits", None), (lab.cpu(), "lits", None), (lab, "lits", "agg"),
                                (lab, "brats", None), (lab, "lits", "mean")):
        with pytest.raises(_lib.EffqError):
            ops.seg_lesions(x, bad_lab, task, fuse)
    with pytest.raises(_lib.EffqError):
        ops.seg_lesions(torch.zeros(9, D, H, W, device=DEV), torch.zeros(9, D, H, W, dtype=torch.uint8, device=DEV),
                        "brats")
    torch.cuda.synchronize()
    assert (labels == 7).all() and (ncomp == 7).all() and (counts == 7).all()


# ---- validate_seg and the ptq mission with --is_cc ------------------------------------------------------------------
def _run(tmp_path, name, task, fuse, is_cc, data_dir, split_dir):
    from efficientq_amd import entrance
    snap = str(tmp_path / name)
    nmod, ncls = ("1", "3") if task == "lits" else ("4", "4")
    argv = ["ptq", "--task", task, "--qconv", "effq", "--qlvl_w", "4", "--qlvl_a", "4", "--q_first", "256,-1",
            "--q_last", "256,-1", "--width", "8,16,8", "--depth", "1,1,1", "--init_stride", "1", "--nMod", nmod,
            "--nClass", ncls, "--blk", "mid", "--ds", "simple", "--hetero_dim", "--drop_rate", "0.5",
            "--lwq_batchsz", "2", "--lwq_patchsz", "16,16,16", "--patch_size", "20,20,18", "--data_dir", data_dir,
            "--split_dir", split_dir, "--test_fp", "--save_nii", "--snap_dir", snap]
    if task == "brats":
        argv += ["--multi_label", "brats", "--merge_type", fuse]
    if is_cc:
        argv.append("--is_cc")
    entrance.main(argv)
    return snap


@pytest.mark.parametrize("task,fuse", [("lits", None), ("brats", "agg"), ("brats", "con")])
def test_mission_with_is_cc_writes_lesion_columns_that_the_maps_reproduce(tmp_path, task, fuse):
    shape = (20, 24, 18)
    val = ["c1", "c0"]
    data_dir, split_dir, arrays = write_dataset(str(tmp_path), task, ["c2", "c0", "c1"], shape, "npy",
                                                train=["c2", "c0"], val=val)
    snap = _run(tmp_path, "with", task, fuse, True, data_dir, split_dir)
    plain = _run(tmp_path, "without", task, fuse, False, data_dir, split_dir)
    head = ("subject", "class") + E.METRICS + ("tp", "fp", "fn", "tn")
    totall = {}
    for folder in ("fp", "ptq"):
        rows = list(csv.reader(open(os.path.join(snap, folder, "metrics.csv"))))
        rows_plain = list(csv.reader(open(os.path.join(plain, folder, "metrics.csv"))))
        assert tuple(rows_plain[0]) == head
        assert tuple(rows[0]) == head + ("totall", "predl", "fnl", "fpl")
        assert [r[:10] for r in rows] == rows_plain
        got = {(r[0], int(r[1])): [int(v) for v in r[10:]] for r in rows[1:]}
        assert len(got) == len(val) * 3
        for sn in val:
            m, _ = read_nifti(os.path.join(snap, folder, "val", f"{sn}.nii.gz"))
            raw = arrays[sn][1]
            if task == "lits":
                pred = [m == c for c in range(3)]
                gt = [raw == c for c in range(3)]
            else:
                pred = [m > 0, (m == 1) | (m == 4), m == 4]
                gt = [raw > 0, (raw == 1) | (raw == 3), raw == 3]
            for c in range(3):
                assert got[(sn, c)] == lesion_counts(pred[c], gt[c]), (folder, sn, c)
                totall.setdefault((sn, c), set()).add(got[(sn, c)][0])
    assert all(len(v) == 1 for v in totall.values())


def test_validate_seg_without_lesions_keeps_its_keys(ops):
    """lesions=False: the dict keys of before; lesions=True: one more key, the same counts."""
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
    loader = [(torch.randn(1, 1, 20, 24, 18, generator=g), torch.randint(0, 3, (1, 20, 24, 18), generator=g))]
    plain = E.validate_seg(model, loader, "lits", (16, 16, 16), 4)
    cc = E.validate_seg(model, loader, "lits", (16, 16, 16), 4, lesions=True)
    assert set(plain[0]) == {"name", "counts", "dsc", "sens", "spec", "acc"}
    assert set(cc[0]) == set(plain[0]) | {"lesions"}
    assert torch.equal(plain[0]["counts"], cc[0]["counts"])
    assert cc[0]["lesions"].shape == (3, 4) and cc[0]["lesions"].dtype == torch.int64
    assert E.lesion_totals(cc).tolist() == cc[0]["lesions"].tolist()
