"""The exact distance transform and the surface-distance metrics on a real MI355X (-m gpu): effq_edt_sq voxel for voxel
against the yardstick of test_seg_surface_cpu (ragged and degenerate extents, a line longer than a workgroup, a site in a
corner, planes with and without sites in one call, three densities, one full-size plane against scipy), effq_seg_surface
against the yardstick on the masks of the torch restatements of test_seg_labels_gpu and on a full-size case known by
construction, its argument checks, validate_seg(surface=True) and the ptq mission with --surf_dist tied back to the label
maps they write.  Every comparison on integers is equality."""
import csv
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, evaluate as E
from efficientq_amd.hip_ops import get_ops
from efficientq_amd.nifti import read_nifti
from tests.test_seg_eval_cpu import write_dataset
from tests.test_seg_labels_gpu import _logits, merge_basic, pred_lits
from tests.test_seg_surface_cpu import (INF, edt_sq_lines, ref_edt_sq, ref_surface, ref_surface_counts,
                                        ref_surface_metrics)

try:
    from scipy import ndimage
except ImportError:
    ndimage = None

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUM_RTOL = 1e-9          # at most 8.9 M correctly rounded terms: n * 2^-53 = 1e-9


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def _edt_twice(ops, masks):
    """edt_sq on a workspace filled with 0xFF, twice: the same bits both times."""
    m = torch.as_tensor(np.ascontiguousarray(masks), dtype=torch.uint8).to(DEV)
    ops.edt_sq(m)                            # sizes the workspace
    ops._ws["surf"].fill_(0xFF)
    sq1 = ops.edt_sq(m).clone()
    ops._ws["surf"].fill_(0xFF)
    sq2 = ops.edt_sq(m)
    assert sq1.dtype == torch.int32 and sq1.shape == m.shape
    assert torch.equal(sq1, sq2)
    return sq1.cpu().numpy()


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _corner(shape):
    m = np.zeros(shape, np.uint8)
    m[-1, -1, -1] = 1
    return m


CASES = {
    "ragged_sparse": lambda: _random((37, 53, 71), 1e-4, 1) | _corner((37, 53, 71)),
    "ragged": lambda: _random((37, 53, 71), 0.02, 2),
    "ragged_dense": lambda: _random((37, 53, 71), 0.5, 3),
    "flat_d": lambda: _random((1, 40, 50), 0.02, 4),
    "flat_w": lambda: _random((40, 50, 1), 0.02, 5),
    "flat_h": lambda: _random((40, 1, 50), 0.02, 6),
    "long_line": lambda: _random((1, 1, 700), 0.01, 7),
    "long_column": lambda: _random((300, 1, 3), 0.01, 8),
    "one_site_in_a_corner": lambda: _corner((9, 33, 70)),
    "full": lambda: np.ones((5, 6, 70), np.uint8),
    "one_voxel": lambda: np.ones((1, 1, 1), np.uint8),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_edt_sq_equals_the_yardstick(ops, case):
    mask = CASES[case]()
    got = _edt_twice(ops, mask)
    want = edt_sq_lines(mask)
    assert np.array_equal(got, want), f"{int((got != want).sum())} voxels differ"
    if mask.size <= 40000:
        assert np.array_equal(got, ref_edt_sq(mask))
    if case == "one_site_in_a_corner":
        assert got[0, 0, 0] == 8 ** 2 + 32 ** 2 + 69 ** 2 == got.max()
    if case == "full":
        assert not got.any()


def test_planes_with_and_without_sites_in_one_call(ops):
    shape = (13, 18, 41)
    masks = np.stack([_random(shape, 0.02, 11), np.zeros(shape, np.uint8), _corner(shape), _random(shape, 0.5, 12)])
    got = _edt_twice(ops, masks)
    assert (got[1] == INF).all()
    for p in (0, 2, 3):
        assert np.array_equal(got[p], edt_sq_lines(masks[p])), p


@pytest.mark.skipif(ndimage is None, reason="the full-size map is compared with scipy's")
def test_full_size_plane_equals_scipy(ops):
    shape = (155, 240, 240)
    d, h, w = np.ogrid[:155, :240, :240]
    ball = ((d - 70) ** 2 + (h - 130) ** 2 + (w - 100) ** 2 <= 40 ** 2)
    sites = ref_surface(ball) | (_random(shape, 1e-5, 13) > 0)
    got = ops.edt_sq(torch.from_numpy(sites.astype(np.uint8)).to(DEV)).cpu().numpy()
    want = np.rint(ndimage.distance_transform_edt(~sites) ** 2).astype(np.int64)
    assert np.array_equal(got, want)


# ---- seg_surface ----------------------------------------------------------------------------------------------------
SHAPE = (12, 20, 40)
WORST = {"sum_rel": 0.0}


def _blocky(shape, nvals, seed, channels=None):
    """Labels made of 2 x 4 x 4 blocks of one value, so that the surfaces are more than dust."""
    g = torch.Generator().manual_seed(seed)
    lead = () if channels is None else (channels,)
    small = torch.randint(0, nvals, lead + (shape[0] // 2, shape[1] // 4, shape[2] // 4), generator=g)
    return small.repeat_interleave(2, -3).repeat_interleave(4, -2).repeat_interleave(4, -1).to(torch.uint8)


def _rel(got, want):
    return abs(got - want) / abs(want) if want else abs(got)


def _check_surface(ops, x, lab, task, fuse, pred, gt, edt=edt_sq_lines):
    counts, sums = ops.seg_surface(x, lab, task, fuse)
    counts, sums = counts.clone(), sums.clone()
    assert counts.dtype == torch.int64 and counts.shape == (x.shape[0], 6)
    assert sums.dtype == torch.float64 and sums.shape == (x.shape[0], 2)
    ops._ws["surf"].fill_(0xFF)
    counts2, sums2 = ops.seg_surface(x, lab, task, fuse)
    assert torch.equal(counts, counts2) and torch.equal(sums.view(torch.int64), sums2.view(torch.int64))
    got = E.surface_metrics(counts, sums, x.shape[1:])
    print(task, fuse, "surface counts", counts.tolist(), "metrics", got.tolist())
    for c in range(x.shape[0]):
        row, want_sums = ref_surface_counts(pred[c], gt[c], edt)
        assert counts[c].tolist() == row, c
        for k in range(2):
            rel = _rel(float(sums[c, k]), want_sums[k])
            WORST["sum_rel"] = max(WORST["sum_rel"], rel)
            assert rel <= SUM_RTOL, (c, k, float(sums[c, k]), want_sums[k])
        want = ref_surface_metrics(pred[c], gt[c], edt)
        for k in range(3):
            assert _rel(float(got[c, k]), want[k]) <= SUM_RTOL, (c, k, got[c].tolist(), want)
    print("worst relative error of a sum so far", WORST["sum_rel"])
    return counts, got


@pytest.mark.parametrize("C", [2, 3, 8])
def test_argmax_surface_equals_the_yardstick(ops, C):
    x = _logits(ops, 1, C, SHAPE, 30 + C, sigmoid=False)[0]            # ties and NaNs
    lab = _blocky(SHAPE, C, 40 + C).to(DEV)
    pred = pred_lits(x[None])[0].cpu().numpy()
    labn = lab.cpu().numpy()
    _check_surface(ops, x, lab, "lits", None, [pred == c for c in range(C)], [labn == c for c in range(C)])


@pytest.mark.parametrize("fuse", [None, "agg", "con"])
@pytest.mark.parametrize("C", [1, 3, 8])
def test_sigmoid_surface_equals_the_yardstick(ops, C, fuse):
    x = _logits(ops, 1, C, SHAPE, 50 + C, sigmoid=True)[0]             # the threshold and 1024 ulps either side of it
    lab = _blocky(SHAPE, 2, 60 + C, channels=C).to(DEV)
    hard = merge_basic((torch.sigmoid(x[None]) >= 0.5).int(), fuse)[0].cpu().numpy()
    _check_surface(ops, x, lab, "brats", fuse, hard, lab.cpu().numpy())


def test_smooth_logits_empty_classes_and_an_unaligned_pointer(ops):
    """Blocky logits: surfaces that are sheets, not dust; class 1 is predicted nowhere, class 2 neither predicted nor
    labelled; the logits start off a 16-byte boundary."""
    g = torch.Generator().manual_seed(3)
    shape = (18, 28, 68)
    small = torch.randn(3, 6, 7, 17, generator=g)
    x = small.repeat_interleave(3, 1).repeat_interleave(4, 2).repeat_interleave(4, 3).contiguous()
    x[1:] = -5.0
    lab = _blocky(shape, 2, 4, channels=3)[:, :18].contiguous()
    lab[2] = 0
    lab = lab.to(DEV)
    buf = torch.empty(1 + x.numel(), device=DEV)
    y = buf[1:].view(x.shape)
    y.copy_(x)
    assert y.data_ptr() % 16 != 0
    hard = merge_basic((torch.sigmoid(y[None]) >= 0.5).int(), None)[0].cpu().numpy()
    counts, got = _check_surface(ops, y, lab, "brats", None, hard, lab.cpu().numpy())
    diag = math.sqrt(18 ** 2 + 28 ** 2 + 68 ** 2)
    assert counts[1, 0] == 0 and counts[1, 1] > 0 and got[1].tolist() == [diag] * 3
    assert counts[2].tolist() == [0] * 6 and got[2].tolist() == [0.0] * 3


def test_full_size_case_known_by_construction(ops):
    """155 x 240 x 240, argmax with two classes: the label is a ball, the prediction the same ball shifted by (3, 4, 0)
    plus one voxel far away.  The island alone sets hd; hd95 does not see it."""
    D, H, W = 155, 240, 240
    d, h, w = np.ogrid[:D, :H, :W]
    gt = ((d - 70) ** 2 + (h - 120) ** 2 + (w - 110) ** 2 <= 30 ** 2)
    pred = ((d - 73) ** 2 + (h - 124) ** 2 + (w - 110) ** 2 <= 30 ** 2)
    island = (150, 235, 236)
    pred[island] = True
    x = torch.from_numpy(np.stack([~pred, pred]).astype(np.float32)).to(DEV)
    lab = torch.from_numpy(gt.astype(np.uint8)).to(DEV)
    counts, sums = ops.seg_surface(x, lab, "lits")
    got = E.surface_metrics(counts, sums, (D, H, W))
    sp, sl = ref_surface(pred), ref_surface(gt)
    far = int(((np.argwhere(sl) - np.array(island)) ** 2).sum(1).min())
    c = counts[1].tolist()
    print("full size", counts.tolist(), got.tolist())
    assert c[0] == int(sp.sum()) and c[1] == int(sl.sum())
    assert c[2] == far and float(got[1, 0]) == math.sqrt(far) > 150
    assert 0 < c[3] <= 25 and c[4] <= c[5] <= 25          # a surface voxel moved by (3, 4, 0) is one of the other ball
    assert 0 < float(got[1, 2]) < float(got[1, 1]) <= 5.0
    # class 0 is the complement: its surfaces are the shells of the volume and of the balls
    assert counts[0, 0] > counts[1, 0] and counts[0, 1] > counts[1, 1]
    if ndimage is not None:
        edt = lambda s: np.rint(ndimage.distance_transform_edt(~s) ** 2).astype(np.int64)
        for k, (p, g) in enumerate(((~pred, ~gt), (pred, gt))):
            row, want_sums = ref_surface_counts(p, g, edt)
            assert counts[k].tolist() == row
            for j in range(2):
                rel = _rel(float(sums[k, j]), want_sums[j])
                print("full size sum", k, j, float(sums[k, j]), want_sums[j], rel)
                assert rel <= SUM_RTOL
            want = ref_surface_metrics(p, g, edt)
            assert all(_rel(float(got[k, j]), want[j]) <= SUM_RTOL for j in range(3))


# ---- argument checks ------------------------------------------------------------------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_argument_errors_leave_the_outputs_untouched(ops):
    D, H, W = 5, 6, 7
    ARG = 1
    assert _lib._ERR_NAMES[ARG] == "EFFQ_ERR_ARG"
    m = torch.ones(D, H, W, dtype=torch.uint8, device=DEV)
    sq = torch.full((D, H, W), 7, dtype=torch.int32, device=DEV)
    need = ops.lib.effq_surf_ws_bytes(1, D, H, W)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    stream = ops.stream
    assert ops.lib.effq_edt_sq(_ptr(m), 1, D, H, W, _ptr(sq), _ptr(ws), need - 1, stream) == ARG
    assert ops.lib.effq_edt_sq(_ptr(m), 1, D, H, W, _ptr(sq), _ptr(ws), 0, stream) == ARG
    assert ops.lib.effq_edt_sq(None, 1, D, H, W, _ptr(sq), _ptr(ws), need, stream) == ARG
    assert ops.lib.effq_edt_sq(_ptr(m), 1, D, H, W, None, _ptr(ws), need, stream) == ARG
    assert ops.lib.effq_edt_sq(_ptr(m), 1, D, H, W, _ptr(sq), None, need, stream) == ARG
    assert ops.lib.effq_edt_sq(_ptr(m), 0, D, H, W, _ptr(sq), _ptr(ws), need, stream) == ARG
    assert ops.lib.effq_edt_sq(_ptr(m), 1, 2048, 1024, 1024, _ptr(sq), _ptr(ws), need, stream) == ARG      # 2^31 voxels
    assert ops.lib.effq_edt_sq(_ptr(m), 1, 1, 1, 46341, _ptr(sq), _ptr(ws), need, stream) == ARG           # W^2 >= 2^31
    with pytest.raises(_lib.EffqError):
        _lib.check(ARG, "effq_edt_sq")
    assert ops.lib.effq_surf_ws_bytes(1, 2048, 1024, 1024) == 0 and ops.lib.effq_surf_ws_bytes(1, 0, 4, 4) == 0
    assert ops.lib.effq_surf_ws_bytes(1, _lib.EDT_MAX_LINE + 1, 1, 1) == 0
    assert ops.lib.effq_surf_ws_bytes(1, 1, 1, 46341) == 0 and ops.lib.effq_surf_ws_bytes(65536, 1, 1, 1) == 0
    x = torch.zeros(3, D, H, W, device=DEV)
    lab = torch.zeros(D, H, W, dtype=torch.uint8, device=DEV)
    counts = torch.full((3, 6), 7, dtype=torch.int64, device=DEV)
    sums = torch.full((3, 2), 7.0, dtype=torch.float64, device=DEV)
    need3 = ops.lib.effq_surf_ws_bytes(6, D, H, W)
    ws3 = torch.zeros(need3, dtype=torch.uint8, device=DEV)

    def call(xp, lp, ncls, mode, fuse, cp, sp, wp, nbytes, dims=(D, H, W)):
        return ops.lib.effq_seg_surface(xp, lp, ncls, *dims, mode, fuse, 0.0, cp, sp, wp, nbytes, stream)
    good = (_ptr(x), _ptr(lab), 3, _lib.SEG_ARGMAX, 0, _ptr(counts), _ptr(sums), _ptr(ws3), need3)
    for k, bad in ((0, None), (1, None), (2, 0), (2, _lib.SEG_TALLIES_MAX_CLASSES + 1), (3, 2), (4, 3), (5, None),
                   (6, None), (7, None), (8, need3 - 1)):
        a = list(good)
        a[k] = bad
        assert call(*a) == ARG, (k, bad)
    assert call(*good, dims=(2048, 1024, 1024)) == ARG
    torch.cuda.synchronize()
    assert (sq == 7).all() and (counts == 7).all() and (sums == 7).all()
    assert call(*good) == 0
    # everything is class 0 in both masks: its surface is the shell of the volume, at distance 0 from itself
    shell = D * H * W - (D - 2) * (H - 2) * (W - 2)
    assert counts.tolist() == [[shell, shell, 0, 0, 0, 0], [0] * 6, [0] * 6] and not sums.any()
    with pytest.raises(_lib.EffqError):
        ops.edt_sq(m.float())
    with pytest.raises(_lib.EffqError):
        ops.edt_sq(m.cpu())
    with pytest.raises(_lib.EffqError):
        ops.edt_sq(m[0])
    for bad_lab, task, fuse in ((lab.float(), "lits", None), (lab.cpu(), "lits", None), (lab, "lits", "agg"),
                                (lab, "brats", None), (lab, "lits", "mean")):
        with pytest.raises(_lib.EffqError):
            ops.seg_surface(x, bad_lab, task, fuse)
    with pytest.raises(_lib.EffqError):
        ops.seg_surface(torch.zeros(9, D, H, W, device=DEV), torch.zeros(9, D, H, W, dtype=torch.uint8, device=DEV),
                        "brats")


# ---- validate_seg and the ptq mission with --surf_dist --------------------------------------------------------------
def _tiny_model():
    from efficientq_amd import calibrate as K, config as Cf, synth
    args = Cf.make_args(Cf.TINY_NET, 4, 4)
    QConv, _, kwQ = Cf.get_conv_class(args)
    model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
    synth.randomise_network(model, 0)
    model.eval()
    K.search_fold_and_remove_bn(model)
    model.to(DEV)
    K.set_fp(model)
    return model


def test_validate_seg_surface_equals_the_yardstick_on_its_own_maps(ops, tmp_path):
    model = _tiny_model()
    g = torch.Generator().manual_seed(1)
    shape = (20, 24, 18)
    loader = [(torch.randn(1, 1, *shape, generator=g), _blocky((20, 24, 20), 3, 5 + k)[None, ..., :18].contiguous())
              for k in range(2)]
    unchanged = E.validate_seg(model, loader, "lits", (16, 16, 16), 4)
    plain = E.validate_seg(model, loader, "lits", (16, 16, 16), 4, surface=False)
    sd = E.validate_seg(model, loader, "lits", (16, 16, 16), 4, surface=True, lesions=True,
                        save_dir=str(tmp_path / "val"), label_dtype=np.uint8)
    assert set(plain[0]) == set(unchanged[0]) == {"name", "counts", "dsc", "sens", "spec", "acc"}
    assert set(sd[0]) == set(plain[0]) | {"lesions", "surface", "surface_counts"}
    E.write_metrics_csv(str(tmp_path / "a.csv"), unchanged)
    E.write_metrics_csv(str(tmp_path / "b.csv"), plain)
    assert open(tmp_path / "a.csv", "rb").read() == open(tmp_path / "b.csv", "rb").read()
    for k, (r, q) in enumerate(zip(sd, plain)):
        assert torch.equal(r["counts"], q["counts"]) and torch.equal(r["counts"], unchanged[k]["counts"])
        assert r["surface"].shape == (3, 3) and r["surface"].dtype == torch.float64
        assert r["surface_counts"].shape == (3, 6) and r["surface_counts"].dtype == torch.int64
        m, _ = read_nifti(str(tmp_path / "val" / f"{k}.nii.gz"))
        raw = loader[k][1][0].numpy()
        for c in range(3):
            row, _ = ref_surface_counts(m == c, raw == c, edt_sq_lines)
            assert r["surface_counts"][c].tolist() == row, (k, c)
            want = ref_surface_metrics(m == c, raw == c, edt_sq_lines)
            assert all(_rel(float(r["surface"][c, j]), want[j]) <= SUM_RTOL for j in range(3)), (k, c)
    means = E.surface_means(sd)
    assert torch.equal(means, (sd[0]["surface"] + sd[1]["surface"]) / 2)


def _run(tmp_path, name, task, fuse, flags, data_dir, split_dir):
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
    entrance.main(argv + list(flags))
    return snap


@pytest.mark.parametrize("task,fuse", [("lits", None), ("brats", "agg")])
def test_mission_with_surf_dist_writes_columns_that_the_maps_reproduce(tmp_path, task, fuse):
    shape = (20, 24, 18)
    val = ["c1", "c0"]
    data_dir, split_dir, arrays = write_dataset(str(tmp_path), task, ["c2", "c0", "c1"], shape, "npy",
                                                train=["c2", "c0"], val=val)
    plain = _run(tmp_path, "without", task, fuse, (), data_dir, split_dir)
    snap = _run(tmp_path, "with", task, fuse, ("--surf_dist",), data_dir, split_dir)
    both = _run(tmp_path, "both", task, fuse, ("--surf_dist", "--is_cc"), data_dir, split_dir)
    head = ("subject", "class") + E.METRICS + ("tp", "fp", "fn", "tn")
    for folder in ("fp", "ptq"):
        rows = list(csv.reader(open(os.path.join(snap, folder, "metrics.csv"))))
        rows_both = list(csv.reader(open(os.path.join(both, folder, "metrics.csv"))))
        rows_plain = list(csv.reader(open(os.path.join(plain, folder, "metrics.csv"))))
        assert tuple(rows_plain[0]) == head
        assert tuple(rows[0]) == head + E.SURFACE_COLUMNS
        assert tuple(rows_both[0]) == head + E.LESION_COLUMNS + E.SURFACE_COLUMNS
        assert [r[:10] for r in rows] == rows_plain == [r[:10] for r in rows_both]
        assert [r[10:] for r in rows] == [r[14:] for r in rows_both]
        got = {(r[0], int(r[1])): [float(v) for v in r[10:]] for r in rows[1:]}
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
                want = ref_surface_metrics(pred[c], gt[c], edt_sq_lines)      # the file holds 7 significant digits
                assert all(abs(a - b) <= 1e-6 * abs(b) for a, b in zip(got[(sn, c)], want)), (folder, sn, c)
