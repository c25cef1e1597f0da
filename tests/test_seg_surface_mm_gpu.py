"""The weighted distance transform and the surface distances in millimetres on a real MI355X (-m gpu): effq_edt_sq_mm bit
for bit against the fp32 yardstick of test_geometry_cpu on the shapes of test_seg_surface_gpu for four spacings, against
effq_edt_sq at unit spacing, effq_seg_surface_mm against the yardstick on the masks of the torch restatements and on a
full-size case whose distances have a closed form in mm, its argument checks, validate_seg(geometry=...) and the ptq
mission with --src_geom / --spacing tied back to the files they write.  fp32 values are compared as bit patterns."""
import csv
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, evaluate as E
from efficientq_amd.hip_ops import get_ops
from efficientq_amd.nifti import read_geometry, read_nifti
from tests.test_geometry_cpu import (SPACINGS, SRC_ROWS, bits, ref_edt_mm_brute, ref_edt_mm_lines,
                                     ref_surface_counts_mm, ref_surface_metrics_mm, weights, write_sources)
from tests.test_seg_eval_cpu import write_dataset
from tests.test_seg_labels_gpu import _logits, merge_basic, pred_lits
from tests.test_seg_surface_gpu import CASES, SUM_RTOL, _blocky, _corner, _random, _rel, _run, _tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
ANISO = (5.0, 0.7421875, 0.7421875)


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def _edt_twice(ops, masks, spacing):
    """edt_sq_mm on a workspace filled with 0xFF, twice: the same bits both times."""
    m = torch.as_tensor(np.ascontiguousarray(masks), dtype=torch.uint8).to(DEV)
    ops.edt_sq_mm(m, spacing)                # sizes the workspace
    ops._ws["surf_mm"].fill_(0xFF)
    sq1 = ops.edt_sq_mm(m, spacing).clone()
    ops._ws["surf_mm"].fill_(0xFF)
    sq2 = ops.edt_sq_mm(m, spacing)
    assert sq1.dtype == torch.float32 and sq1.shape == m.shape
    assert torch.equal(sq1.view(torch.int32), sq2.view(torch.int32))
    return sq1.cpu().numpy()


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_edt_sq_mm_equals_the_yardstick_bit_for_bit(ops, case, spacing):
    mask = CASES[case]()
    got = _edt_twice(ops, mask, spacing)
    want = ref_edt_mm_lines(mask, spacing)
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{int(diff.sum())} voxels differ, first {got[diff][:3]} against {want[diff][:3]}"
    if mask.size <= 3000:
        assert np.array_equal(bits(got), bits(ref_edt_mm_brute(mask, spacing)))
    if case == "one_site_in_a_corner":
        wd, wh, ww = weights(spacing)
        assert got[0, 0, 0] == (ww * F32(69 ** 2) + wh * F32(32 ** 2)) + wd * F32(8 ** 2) == got.max()
    if case == "full":
        assert not got.any()


@pytest.mark.parametrize("spacing", SPACINGS)
def test_planes_with_and_without_sites_in_one_call(ops, spacing):
    shape = (13, 18, 41)
    masks = np.stack([_random(shape, 0.02, 11), np.zeros(shape, np.uint8), _corner(shape), _random(shape, 0.5, 12)])
    got = _edt_twice(ops, masks, spacing)
    assert np.isposinf(got[1]).all()
    for p in (0, 2, 3):
        assert np.array_equal(bits(got[p]), bits(ref_edt_mm_lines(masks[p], spacing))), p


@pytest.mark.parametrize("case", sorted(CASES))
def test_unit_spacing_equals_the_integer_transform(ops, case):
    mask = CASES[case]()
    m = torch.from_numpy(mask).to(DEV)
    masks = torch.stack([m, torch.zeros_like(m)])
    got, want = ops.edt_sq_mm(masks, (1, 1, 1)), ops.edt_sq(masks)
    assert torch.equal(got[0], want[0].float()) and torch.equal(got[0].to(torch.int32), want[0])
    assert torch.isposinf(got[1]).all() and (want[1] == np.iinfo(np.int32).max).all()


# ---- seg_surface_mm -------------------------------------------------------------------------------------------------
SHAPE = (12, 20, 40)
WORST = {"sum_rel": 0.0}


def _check_surface_mm(ops, x, lab, task, fuse, pred, gt, spacing, edt=ref_edt_mm_lines):
    counts, sq, sums = (t.clone() for t in ops.seg_surface_mm(x, lab, task, fuse, spacing))
    Cc = x.shape[0]
    assert counts.dtype == torch.int64 and counts.shape == (Cc, 2)
    assert sq.dtype == torch.float32 and sq.shape == (Cc, 4)
    assert sums.dtype == torch.float64 and sums.shape == (Cc, 2)
    ops._ws["surf_mm"].fill_(0xFF)
    counts2, sq2, sums2 = ops.seg_surface_mm(x, lab, task, fuse, spacing)
    assert torch.equal(counts, counts2) and torch.equal(sq.view(torch.int32), sq2.view(torch.int32))
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64))
    got = E.surface_metrics_mm(counts, sq, sums, x.shape[1:], spacing)
    print(task, fuse, spacing, "counts", counts.tolist(), "sq", sq.tolist(), "metrics", got.tolist())
    for c in range(Cc):
        cnt, want_sq, want_sums = ref_surface_counts_mm(pred[c], gt[c], spacing, edt)
        assert counts[c].tolist() == cnt, c
        assert np.array_equal(bits(sq[c].cpu().numpy()), bits(np.array(want_sq, F32))), (c, sq[c].tolist(), want_sq)
        for k in range(2):
            rel = _rel(float(sums[c, k]), want_sums[k])
            WORST["sum_rel"] = max(WORST["sum_rel"], rel)
            assert rel <= SUM_RTOL, (c, k, float(sums[c, k]), want_sums[k])
        want = ref_surface_metrics_mm(pred[c], gt[c], spacing, edt)
        for k in range(3):
            assert _rel(float(got[c, k]), want[k]) <= SUM_RTOL, (c, k, got[c].tolist(), want)
    print("worst relative error of a sum so far", WORST["sum_rel"])
    return counts, sq, sums, got


@pytest.mark.parametrize("spacing", SPACINGS[1:])
@pytest.mark.parametrize("C", [2, 3, 8])
def test_argmax_surface_mm_equals_the_yardstick(ops, C, spacing):
    x = _logits(ops, 1, C, SHAPE, 30 + C, sigmoid=False)[0]            # ties and NaNs
    lab = _blocky(SHAPE, C, 40 + C).to(DEV)
    pred = pred_lits(x[None])[0].cpu().numpy()
    labn = lab.cpu().numpy()
    _check_surface_mm(ops, x, lab, "lits", None, [pred == c for c in range(C)], [labn == c for c in range(C)], spacing)


@pytest.mark.parametrize("fuse", [None, "agg", "con"])
@pytest.mark.parametrize("C", [1, 3, 8])
def test_sigmoid_surface_mm_equals_the_yardstick(ops, C, fuse):
    x = _logits(ops, 1, C, SHAPE, 50 + C, sigmoid=True)[0]             # the threshold and 1024 ulps either side of it
    lab = _blocky(SHAPE, 2, 60 + C, channels=C).to(DEV)
    hard = merge_basic((torch.sigmoid(x[None]) >= 0.5).int(), fuse)[0].cpu().numpy()
    for spacing in (ANISO, SPACINGS[3]):
        _check_surface_mm(ops, x, lab, "brats", fuse, hard, lab.cpu().numpy(), spacing)


def _mask_logits(pred, gt):
    """Argmax logits and label of two classes whose class 1 is `pred` / `gt`."""
    x = torch.from_numpy(np.stack([~pred, pred]).astype(np.float32)).to(DEV)
    return x, torch.from_numpy(gt.astype(np.uint8)).to(DEV)


@pytest.mark.parametrize("k", [20, 21, 40, 7])
def test_pooled_ranks_on_and_off_an_order_statistic(ops, k):
    """k isolated voxels at growing distances from a single voxel: n = k + 1 pooled values in class 1; 95 (n - 1) is a
    multiple of 100 for k = 20 and k = 40 and is not for the others."""
    shape = (3, 90, 8)
    one = np.zeros(shape, bool)
    one[1, 0, 0] = True
    many = np.zeros(shape, bool)
    for i in range(k):
        many[1, 2 * i + 3, 3 * i % 8] = True
    x, lab = _mask_logits(many, one)
    for spacing in (ANISO, SPACINGS[2]):
        counts, sq, _, _ = _check_surface_mm(ops, x, lab, "lits", None, [~many, many], [~one, one], spacing)
        n = int(counts[1].sum())
        assert n == k + 1 and (95 * (n - 1) % 100 == 0) == (k in (20, 40))
        assert float(sq[1, 2]) <= float(sq[1, 3]) <= float(sq[1, :2].max())


def test_unit_spacing_gives_the_hd_and_hd95_of_the_integer_path(ops):
    x = _logits(ops, 1, 3, SHAPE, 71, sigmoid=True)[0]
    lab = _blocky(SHAPE, 2, 72, channels=3).to(DEV)
    old_c, old_s = ops.seg_surface(x, lab, "brats", "agg")
    counts, sq, sums = ops.seg_surface_mm(x, lab, "brats", "agg", (1, 1, 1))
    assert torch.equal(counts, old_c[:, :2])
    assert torch.equal(sq, old_c[:, 2:].float()) and torch.equal(sq.to(torch.int64), old_c[:, 2:])
    old = E.surface_metrics(old_c, old_s, SHAPE)
    new = E.surface_metrics_mm(counts, sq, sums, SHAPE, (1, 1, 1))
    assert torch.equal(new[:, :2], old[:, :2])
    for c in range(3):
        for k in range(2):
            assert _rel(float(sums[c, k]), float(old_s[c, k])) <= SUM_RTOL
        assert _rel(float(new[c, 2]), float(old[c, 2])) <= SUM_RTOL


def _shell(lo, hi, shape):
    m = np.zeros(shape, bool)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    inner = np.zeros(shape, bool)
    inner[lo[0] + 1:hi[0] - 1, lo[1] + 1:hi[1] - 1, lo[2] + 1:hi[2] - 1] = True
    return m, np.argwhere(m & ~inner)


def _to_box_shell(v, lo, hi, w):
    """E of the voxels v (n x 3) to the shell of the box lo:hi in the kernel's fp32 arithmetic, in closed form: outside
    the box the nearest shell voxel is v clamped into it (every |component| is least at once); inside, the nearest face
    along one axis (every shell voxel is at least that far along the axis whose face it lies on)."""
    cl = np.clip(v, lo, np.array(hi) - 1)
    d2 = ((v - cl) ** 2).astype(F32)
    out = (w[2] * d2[:, 2] + w[1] * d2[:, 1]) + w[0] * d2[:, 0]
    inside = (v == cl).all(1)
    face = np.minimum(v - np.array(lo), np.array(hi) - 1 - v)
    e_in = np.min(np.stack([w[a] * (face[:, a] ** 2).astype(F32) for a in range(3)]), 0)
    return np.where(inside, e_in, out).astype(F32)


def test_full_size_case_known_by_construction(ops):
    """3 classes, 155 x 240 x 240, spacing (5, 0.7421875, 0.7421875) mm: each label is a box and each prediction the
    same box shifted, along d alone, in the plane alone, and along all three axes."""
    shape = (155, 240, 240)
    w = weights(ANISO)
    boxes = [((40, 60, 70), (100, 170, 180), (1, 0, 0)), ((50, 80, 90), (90, 150, 160), (0, 3, 4)),
             ((60, 100, 100), (80, 130, 140), (2, 5, 1))]
    x = torch.full((3,) + shape, -1.0)
    lab = torch.zeros((3,) + shape, dtype=torch.uint8)
    want = []
    for c, (lo, hi, sh) in enumerate(boxes):
        plo, phi = tuple(a + s for a, s in zip(lo, sh)), tuple(a + s for a, s in zip(hi, sh))
        gt, s_l = _shell(lo, hi, shape)
        pr, s_p = _shell(plo, phi, shape)
        x[c][torch.from_numpy(pr)] = 1.0
        lab[c][torch.from_numpy(gt)] = 1
        e_pl, e_lp = _to_box_shell(s_p, lo, hi, w), _to_box_shell(s_l, plo, phi, w)
        pooled = np.sort(np.hstack([e_pl, e_lp]))
        n = len(pooled)
        k = 95 * (n - 1) // 100
        want.append(([len(s_p), len(s_l)], np.array([e_pl.max(), e_lp.max(), pooled[k], pooled[min(k + 1, n - 1)]], F32),
                     [float(np.sqrt(e_pl.astype(np.float64)).sum()), float(np.sqrt(e_lp.astype(np.float64)).sum())]))
    counts, sq, sums = ops.seg_surface_mm(x.to(DEV), lab.to(DEV), "brats", None, ANISO)
    got = E.surface_metrics_mm(counts, sq, sums, shape, ANISO)
    print("full size", counts.tolist(), sq.tolist(), sums.tolist(), got.tolist())
    for c, (cnt, wsq, wsum) in enumerate(want):
        assert counts[c].tolist() == cnt, c
        assert np.array_equal(bits(sq[c].cpu().numpy()), bits(wsq)), (c, sq[c].tolist(), wsq.tolist())
        for k in range(2):
            rel = _rel(float(sums[c, k]), wsum[k])
            print("full size sum", c, k, float(sums[c, k]), wsum[k], rel)
            assert rel <= SUM_RTOL
    assert float(got[0, 0]) == 5.0                               # one slice
    assert float(got[1, 0]) == math.sqrt(float((w[2] * F32(16) + w[1] * F32(9)) + w[0] * F32(0)))
    assert abs(float(got[1, 0]) - 5 * 0.7421875) < 1e-6          # 3-4-5 in the plane
    assert float(got[2, 0]) == math.sqrt(float((w[2] * F32(1) + w[1] * F32(25)) + w[0] * F32(4)))


# ---- argument checks ------------------------------------------------------------------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_argument_errors_leave_the_outputs_untouched(ops):
    D, H, W = 5, 6, 7
    ARG = 1
    assert _lib._ERR_NAMES[ARG] == "EFFQ_ERR_ARG"
    lib, stream = ops.lib, ops.stream
    m = torch.ones(D, H, W, dtype=torch.uint8, device=DEV)
    out = torch.full((D, H, W), 7.0, dtype=torch.float32, device=DEV)
    need = lib.effq_surf_mm_ws_bytes(1, D, H, W)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def edt(mp=_ptr(m), P=1, dims=(D, H, W), wts=(1.0, 1.0, 1.0), op=_ptr(out), wp=_ptr(ws), nbytes=need):
        return lib.effq_edt_sq_mm(mp, P, *dims, *wts, op, wp, nbytes, stream)
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        for k in range(3):
            wts = [1.0, 1.0, 1.0]
            wts[k] = bad
            assert edt(wts=wts) == ARG, (bad, k)
    assert edt(nbytes=need - 1) == ARG and edt(nbytes=0) == ARG
    assert edt(mp=None) == ARG and edt(op=None) == ARG and edt(wp=None) == ARG and edt(P=0) == ARG
    for dims in ((4097, 1, 1), (1, 4097, 1), (1, 1, 4097), (2048, 1024, 1024), (0, 4, 4)):
        assert edt(dims=dims) == ARG, dims
        assert lib.effq_surf_mm_ws_bytes(1, *dims) == 0, dims
    assert lib.effq_surf_mm_ws_bytes(65536, 1, 1, 1) == 0 and lib.effq_surf_mm_ws_bytes(1, 4096, 1, 1) > 0
    x = torch.zeros(3, D, H, W, device=DEV)
    lab = torch.zeros(D, H, W, dtype=torch.uint8, device=DEV)
    counts = torch.full((3, 2), 7, dtype=torch.int64, device=DEV)
    sq = torch.full((3, 4), 7.0, dtype=torch.float32, device=DEV)
    sums = torch.full((3, 2), 7.0, dtype=torch.float64, device=DEV)
    need3 = lib.effq_surf_mm_ws_bytes(6, D, H, W)
    ws3 = torch.zeros(need3, dtype=torch.uint8, device=DEV)

    def call(xp, lp, ncls, mode, fuse, wd, wh, ww, cp, qp, sp, wp, nbytes, dims=(D, H, W)):
        return lib.effq_seg_surface_mm(xp, lp, ncls, *dims, mode, fuse, 0.0, wd, wh, ww, cp, qp, sp, wp, nbytes, stream)
    good = (_ptr(x), _ptr(lab), 3, _lib.SEG_ARGMAX, 0, 25.0, 0.5, 0.5, _ptr(counts), _ptr(sq), _ptr(sums), _ptr(ws3),
            need3)
    for k, bad in ((0, None), (1, None), (2, 0), (2, _lib.SEG_TALLIES_MAX_CLASSES + 1), (3, 2), (4, 3), (5, 0.0),
                   (6, -0.5), (7, float("nan")), (5, float("inf")), (8, None), (9, None), (10, None), (11, None),
                   (12, need3 - 1)):
        a = list(good)
        a[k] = bad
        assert call(*a) == ARG, (k, bad)
    assert call(*good, dims=(4097, 1, 1)) == ARG and call(*good, dims=(1, 1, 4097)) == ARG
    torch.cuda.synchronize()
    assert (out == 7).all() and (counts == 7).all() and (sq == 7).all() and (sums == 7).all()
    assert call(*good) == 0
    shell = D * H * W - (D - 2) * (H - 2) * (W - 2)
    assert counts.tolist() == [[shell, shell], [0, 0], [0, 0]] and not sq.any() and not sums.any()
    for bad in ((0, 1, 1), (1, -1, 1), (1, 1, float("nan")), (float("inf"), 1, 1), (1, 1), "1,1,1", None, (1e-30, 1, 1)):
        with pytest.raises(_lib.EffqError):
            ops.edt_sq_mm(m, bad)
        with pytest.raises(_lib.EffqError):
            ops.seg_surface_mm(x, lab, "lits", None, bad)
    with pytest.raises(_lib.EffqError):
        ops.edt_sq_mm(m.float(), (1, 1, 1))
    with pytest.raises(_lib.EffqError):
        ops.edt_sq_mm(m.cpu(), (1, 1, 1))
    with pytest.raises(_lib.EffqError):
        ops.edt_sq_mm(torch.ones(1, 1, 4097, dtype=torch.uint8, device=DEV), (1, 1, 1))
    for bad_lab, task, fuse in ((lab.float(), "lits", None), (lab.cpu(), "lits", None), (lab, "lits", "agg"),
                                (lab, "brats", None), (lab, "lits", "mean")):
        with pytest.raises(_lib.EffqError):
            ops.seg_surface_mm(x, bad_lab, task, fuse, (1, 1, 1))


# ---- validate_seg and the ptq mission -------------------------------------------------------------------------------
def test_validate_seg_with_a_geometry_equals_the_yardstick_on_its_own_maps(ops, tmp_path):
    model = _tiny_model()
    g = torch.Generator().manual_seed(1)
    shape = (20, 24, 18)
    loader = [(torch.randn(1, 1, *shape, generator=g), _blocky((20, 24, 20), 3, 5 + k)[None, ..., :18].contiguous())
              for k in range(2)]
    plain = E.validate_seg(model, loader, "lits", (16, 16, 16), 4)
    vox = E.validate_seg(model, loader, "lits", (16, 16, 16), 4, surface=True)
    per_case = [{"spacing": ANISO}, {"spacing": SPACINGS[3]}]
    mm = E.validate_seg(model, loader, "lits", (16, 16, 16), 4, surface=True, geometry=per_case,
                        save_dir=str(tmp_path / "val"), label_dtype=np.uint8)
    one = E.validate_seg(model, loader, "lits", (16, 16, 16), 4, surface=True, geometry=ANISO)
    assert "surface_unit" not in vox[0] and set(plain[0]) == {"name", "counts", "dsc", "sens", "spec", "acc"}
    assert set(mm[0]) == set(plain[0]) | {"surface", "surface_counts", "surface_sq", "surface_unit"}
    assert torch.equal(one[0]["surface"], mm[0]["surface"]) and not torch.equal(one[1]["surface"], mm[1]["surface"])
    for k, r in enumerate(mm):
        assert torch.equal(r["counts"], plain[k]["counts"]) and r["surface_unit"] == "mm"
        assert torch.equal(r["surface_counts"], vox[k]["surface_counts"][:, :2])
        m, f = read_nifti(str(tmp_path / "val" / f"{k}.nii.gz"))
        assert np.array_equal(f["affine"], np.eye(4))              # a spacing alone moves no file
        raw = loader[k][1][0].numpy()
        for c in range(3):
            cnt, sq, _ = ref_surface_counts_mm(m == c, raw == c, per_case[k]["spacing"])
            assert r["surface_counts"][c].tolist() == cnt
            assert np.array_equal(bits(r["surface_sq"][c].numpy()), bits(np.array(sq, F32)))
            want = ref_surface_metrics_mm(m == c, raw == c, per_case[k]["spacing"])
            assert all(_rel(float(r["surface"][c, j]), want[j]) <= SUM_RTOL for j in range(3)), (k, c)
    E.write_metrics_csv(str(tmp_path / "mm.csv"), mm)
    assert list(csv.reader(open(tmp_path / "mm.csv")))[0][10:] == list(E.SURFACE_COLUMNS_MM)


@pytest.mark.parametrize("task,fuse", [("lits", None), ("brats", "agg")])
def test_mission_with_src_geom_writes_mm_columns_and_maps_on_the_source_grid(tmp_path, task, fuse):
    shape, src_shape, pmin = (20, 24, 18), (24, 26, 21), (2, 1, 3)
    pmax = tuple(a + n for a, n in zip(pmin, shape))
    val = ["c1", "c0"]
    data_dir, split_dir, arrays = write_dataset(str(tmp_path), task, ["c2", "c0", "c1"], shape, "npy",
                                                train=["c2", "c0"], val=val)
    write_sources(data_dir, val, src_shape, crop={sn: (pmin, pmax) for sn in val})
    spacing = (0.7421875, 0.7421875, 5.0)                        # the column norms of SRC_ROWS: array axes 0, 1, 2
    plain = _run(tmp_path, "without", task, fuse, (), data_dir, split_dir)
    snap = _run(tmp_path, "geom", task, fuse, ("--surf_dist", "--src_geom"), data_dir, split_dir)
    alone = _run(tmp_path, "spacing", task, fuse, ("--surf_dist", "--spacing", "0.7421875,0.7421875,5"), data_dir,
                 split_dir)
    head = ("subject", "class") + E.METRICS + ("tp", "fp", "fn", "tn")
    for folder in ("fp", "ptq"):
        rows = list(csv.reader(open(os.path.join(snap, folder, "metrics.csv"))))
        rows_alone = list(csv.reader(open(os.path.join(alone, folder, "metrics.csv"))))
        rows_plain = list(csv.reader(open(os.path.join(plain, folder, "metrics.csv"))))
        assert tuple(rows_plain[0]) == head
        assert tuple(rows[0]) == head + E.SURFACE_COLUMNS_MM == tuple(rows_alone[0])
        assert [r[:10] for r in rows] == rows_plain
        assert rows_alone == rows                                 # the same spacing, given by hand
        got = {(r[0], int(r[1])): r[10:] for r in rows[1:]}
        assert len(got) == len(val) * 3
        for sn in val:
            path = os.path.join(snap, folder, "val", f"{sn}.nii.gz")
            full, f = read_nifti(path)
            g, src = read_geometry(path), read_geometry(os.path.join(data_dir, "src", f"{sn}.nii.gz"))
            assert full.shape == src_shape == src["shape"] and full.dtype == np.uint16
            assert np.array_equal(g["affine"], src["affine"]) and np.array_equal(g["affine"][:3], np.array(SRC_ROWS))
            for k in ("pixdim", "xyzt_units", "qform_code", "sform_code", "quatern", "srow_x", "srow_y", "srow_z"):
                assert g[k] == src[k], k
            assert g["spacing"] == spacing
            m = full[pmin[0]:pmax[0], pmin[1]:pmax[1], pmin[2]:pmax[2]]
            assert full.sum() == m.sum()                          # zeros outside the crop
            cropped, fa = read_nifti(os.path.join(alone, folder, "val", f"{sn}.nii.gz"))
            assert np.array_equal(cropped, m) and np.array_equal(fa["affine"], np.eye(4))
            assert fa["pixdim"] == (1.0,) * 8
            raw = arrays[sn][1]
            if task == "lits":
                pred = [m == c for c in range(3)]
                gt = [raw == c for c in range(3)]
            else:
                pred = [m > 0, (m == 1) | (m == 4), m == 4]
                gt = [raw > 0, (raw == 1) | (raw == 3), raw == 3]
            for c in range(3):
                want = ref_surface_metrics_mm(pred[c], gt[c], spacing)
                assert got[(sn, c)] == ["%.7g" % v for v in want], (folder, sn, c, got[(sn, c)], want)
