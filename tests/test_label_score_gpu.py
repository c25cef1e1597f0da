"""effq_label_lesions and effq_label_surface_mm on a real MI355X (-m gpu): against the entry points that take logits on
one-hot logits (counts, the bits of sq and of the fp64 sums), against the yardsticks of test_geometry_cpu and the
component restatement of test_seg_lesions_cpu on nested classes, `within` against the fp32 distances of the yardstick
(<= on a realised distance), the shapes at which the two new kernels take another path, empty classes, determinism, the
argument checks, and the score mission tied back to the files it writes.  Integers and bit patterns are compared exactly;
the one tolerance is SUM_RTOL of test_seg_surface_gpu for the fp64 sums against the yardstick's."""
import csv
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, entrance, evaluate as E, score
from efficientq_amd.hip_ops import get_ops
from efficientq_amd.ops_score import label_lesions, label_surface_mm, tolerances_sq
from tests.test_geometry_cpu import (SPACINGS, bits, ref_edt_mm_lines, ref_surface_counts_mm, ref_surface_metrics_mm,
                                     weights)
from tests.test_score_cpu import SPACING as FILE_SPACING, blobs, f32_ratios, g7, ref_within, tol_sq, write_pairs
from tests.test_seg_lesions_cpu import lesion_counts
from tests.test_seg_surface_cpu import ref_surface
from tests.test_seg_surface_gpu import SUM_RTOL, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
ANISO = (5.0, 0.7421875, 0.7421875)
SHAPE = (12, 20, 40)
BRATS = Cf.SCORE_CLASSES["brats"]
LITS = Cf.SCORE_CLASSES["lits"]
TOLS8 = (0.0, 0.5, 0.7421875, 1.0, 2.0, 5.0, 7.3, 1000.0)


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def blocky(shape, values, seed):
    """A uint8 map of blocks of 2 x 4 x 4 voxels of one of `values` each, cropped to `shape`."""
    g = np.random.default_rng(seed)
    small = g.integers(0, len(values), size=tuple(-(-n // b) for n, b in zip(shape, (2, 4, 4))))
    a = np.asarray(values, np.uint8)[small].repeat(2, 0).repeat(4, 1).repeat(4, 2)
    return np.ascontiguousarray(a[:shape[0], :shape[1], :shape[2]])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def argmax_lut(Cc):
    return [1 << c for c in range(Cc)] + [0] * (256 - Cc)


@functools.lru_cache(maxsize=None)
def reference(shape, classes, spacing, seeds, tols=()):
    """(pred, truth, per class: counts, sq, sums, lesion counts, within) of two blocky maps, from the yardsticks; computed
    once per case and shared."""
    values = sorted({0} | {v for labels in classes for v in labels})
    pred, truth = blocky(shape, values, seeds[0]), blocky(shape, values, seeds[1])
    per = []
    for labels in classes:
        p, t = np.isin(pred, labels), np.isin(truth, labels)
        per.append((*ref_surface_counts_mm(p, t, spacing), lesion_counts(p, t), ref_within(p, t, spacing, tols)))
    return pred, truth, per


def check_against(ops, pred, truth, classes, spacing, per, tols=()):
    """Both entry points against the per-class reference: integers and fp32 bits exactly, the sums within SUM_RTOL."""
    lut, Cc = Cf.score_class_lut(classes), len(classes)
    counts, sq, sums, within = label_surface_mm(ops, pred, truth, lut, Cc, spacing, tols)
    lesions = label_lesions(ops, pred, truth, lut, Cc)
    assert counts.dtype == torch.int64 and counts.shape == (Cc, 2) and sq.dtype == torch.float32 and sq.shape == (Cc, 4)
    assert sums.dtype == torch.float64 and sums.shape == (Cc, 2) and lesions.dtype == torch.int64
    assert within.dtype == torch.int64 and within.shape == (Cc, 2, len(tols)) and lesions.shape == (Cc, 4)
    for c, (cnt, want_sq, want_sums, want_les, want_within) in enumerate(per):
        assert counts[c].tolist() == cnt, c
        assert np.array_equal(bits(sq[c].cpu().numpy()), bits(np.array(want_sq, F32))), (c, sq[c].tolist(), want_sq)
        for k in range(2):
            rel = _rel(float(sums[c, k]), want_sums[k])
            print("class", c, "sum", k, float(sums[c, k]), want_sums[k], "rel", rel)
            assert rel <= SUM_RTOL, (c, k)
        assert lesions[c].tolist() == want_les, c
        assert within[c].tolist() == [list(w) for w in want_within], (c, within[c].tolist(), want_within)
    return counts, sq, sums, within, lesions


# ---- 1. against the entry points that take logits -------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", SPACINGS[1:])
@pytest.mark.parametrize("Cc", [2, 3, 8])
def test_classes_equal_to_ids_give_the_bits_of_the_logit_entry_points(ops, Cc, spacing):
    pred, lab = dev(blocky(SHAPE, range(Cc), 10 + Cc)), dev(blocky(SHAPE, range(Cc), 20 + Cc))
    x = torch.nn.functional.one_hot(pred.long(), Cc).permute(3, 0, 1, 2).float().contiguous()
    want_c, want_sq, want_s = (t.clone() for t in ops.seg_surface_mm(x, lab, "lits", None, spacing))
    want_l = ops.seg_lesions(x, lab, "lits").clone()
    counts, sq, sums, within = label_surface_mm(ops, pred, lab, argmax_lut(Cc), Cc, spacing)
    assert torch.equal(counts, want_c) and counts.sum() > 0
    assert torch.equal(sq.view(torch.int32), want_sq.view(torch.int32))
    assert torch.equal(sums.view(torch.int64), want_s.view(torch.int64))
    assert within.shape == (Cc, 2, 0)
    assert torch.equal(label_lesions(ops, pred, lab, argmax_lut(Cc), Cc), want_l) and want_l.sum() > 0
    # and with tolerances the first three outputs stay what they were
    counts2, sq2, sums2, within2 = label_surface_mm(ops, pred, lab, argmax_lut(Cc), Cc, spacing, (1.0, 1000.0))
    assert torch.equal(counts2, want_c) and torch.equal(sq2.view(torch.int32), want_sq.view(torch.int32))
    assert torch.equal(sums2.view(torch.int64), want_s.view(torch.int64))
    assert torch.equal(within2[:, :, 1], want_c) and (within2[:, :, 0] <= within2[:, :, 1]).all()


# ---- 2. nested classes ------------------------------------------------------------------------------------------------------
def test_nested_brats_classes_equal_the_yardsticks(ops):
    pred, truth, per = reference(SHAPE, BRATS, ANISO, (31, 32))
    assert {0, 1, 2, 4} == set(np.unique(pred)) == set(np.unique(truth))
    counts, _, _, _, lesions = check_against(ops, dev(pred), dev(truth), BRATS, ANISO, per)
    lut = Cf.score_class_lut(BRATS)
    assert lut == E.post_class_lut("brats", 3)
    tallies = ops.label_tallies(dev(pred), dev(truth), lut, 3)
    for c, labels in enumerate(BRATS):
        p, t = np.isin(pred, labels), np.isin(truth, labels)
        assert tallies[c].tolist() == [int((p & t).sum()), int((p & ~t).sum()), int((~p & t).sum()), int((~p & ~t).sum())]


# ---- 3. within against the yardstick ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tols", [(0.7421875,), TOLS8], ids=["ntol1", "ntol8"])
def test_within_equals_the_yardstick_for_every_class_and_direction(ops, tols):
    pred, truth, per = reference(SHAPE, BRATS, ANISO, (41, 42), tols)
    counts, sq, _, within, _ = check_against(ops, dev(pred), dev(truth), BRATS, ANISO, per, tols)
    k = tols.index(0.7421875)
    t = tol_sq(0.7421875)
    assert t == weights(ANISO)[2]                        # one step along w: a realised distance
    for c, labels in enumerate(BRATS):
        p, l = np.isin(pred, labels), np.isin(truth, labels)
        sp, sl = ref_surface(p), ref_surface(l)
        e_pl, e_lp = ref_edt_mm_lines(sl, ANISO)[sp], ref_edt_mm_lines(sp, ANISO)[sl]
        assert (e_pl == t).any() and (e_lp == t).any()   # <= and < differ on these masks
        assert within[c, 0, k] == int((e_pl <= t).sum()) > int((e_pl < t).sum())
        assert within[c, 1, k] == int((e_lp <= t).sum()) > int((e_lp < t).sum())
    if len(tols) == 8:
        hd_sq = float(sq[:, :2].max())
        assert tol_sq(7.3) not in np.unique(e_pl) and float(tol_sq(1000.0)) > hd_sq
        assert torch.equal(within[:, :, 7], counts)      # above hd: every surface voxel
        assert (within[:, :, 1:] >= within[:, :, :-1]).all() and (within[:, :, 0] < within[:, :, 7]).all()


# ---- 4. shapes where the kernels can go wrong ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7, 67), (1, 9, 130)], ids=["odd_S_two_chunks", "one_slice"])
def test_odd_and_flat_shapes_equal_the_yardsticks(ops, shape):
    tols = (0.0, 0.7421875, 3.0)
    pred, truth, per = reference(shape, LITS, ANISO, (51, 52), tols)
    assert int(np.prod(shape)) % 4 != 0 and (shape[0] == 1 or shape[2] > 64)      # both run the tail of the 4-voxel loops
    check_against(ops, dev(pred), dev(truth), LITS, ANISO, per, tols)


def test_a_map_one_byte_off_a_four_byte_boundary_takes_the_scalar_path(ops):
    shape, tols = (3, 4, 8), (0.0, 1.0)
    pred, truth, per = reference(shape, LITS, SPACINGS[2], (61, 62), tols)
    n = int(np.prod(shape))

    def one_off(a):
        buf = torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
        off = buf[1:1 + n].view(shape)
        off.copy_(dev(a))
        assert off.data_ptr() % 4 == 1 and off.is_contiguous()
        return off
    aligned = check_against(ops, dev(pred), dev(truth), LITS, SPACINGS[2], per, tols)
    for p, t in ((one_off(pred), dev(truth)), (dev(pred), one_off(truth)), (one_off(pred), one_off(truth))):
        got = check_against(ops, p, t, LITS, SPACINGS[2], per, tols)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(aligned, got))


def _brute(points, sites, w):
    """min over the sites of fl(fl(fl(ww dw^2) + fl(wh dh^2)) + fl(wd dd^2)) for every point, in numpy fp32."""
    d2 = ((points[:, None, :] - sites[None, :, :]) ** 2).astype(F32)
    e = (w[2] * d2[..., 2] + w[1] * d2[..., 1]) + w[0] * d2[..., 0]
    assert e.dtype == F32
    return e.min(1)


def test_a_sparse_case_above_the_cap_of_the_streaming_grid(ops):
    """40 x 330 x 330 = 4 356 000 voxels = 1 089 000 groups of 4 = 4254 workgroups of 256: above the cap of 4096, the
    grid-stride loops of k_label_bits and k_surf_within make a second trip, and the last box lies in it."""
    shape = (40, 330, 330)
    assert -(-int(np.prod(shape)) // 4 // 256) > 4096
    boxes_l = [((2, 10, 10), (6, 16, 17)), ((20, 100, 200), (23, 108, 205)), ((37, 320, 318), (40, 327, 326)),
               ((10, 300, 20), (12, 303, 24))]
    boxes_p = [((2, 11, 12), (6, 17, 19)), ((21, 100, 203), (24, 108, 208)), ((37, 321, 319), (40, 328, 327)),
               ((30, 30, 300), (32, 34, 303))]                     # three shifted, the fourth elsewhere
    pred, truth = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for m, boxes in ((pred, boxes_p), (truth, boxes_l)):
        for lo, hi in boxes:
            m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    assert np.flatnonzero(truth)[-1] > 4096 * 256 * 4
    tols = (0.7421875, 2.0, 1000.0)
    counts, sq, sums, within = label_surface_mm(ops, dev(pred), dev(truth), [0, 1] + [0] * 254, 1, ANISO, tols)
    lesions = label_lesions(ops, dev(pred), dev(truth), [0, 1] + [0] * 254, 1)
    sp, sl = np.argwhere(ref_surface(pred)), np.argwhere(ref_surface(truth))
    w = weights(ANISO)
    e_pl, e_lp = _brute(sp, sl, w), _brute(sl, sp, w)
    assert counts.tolist() == [[len(sp), len(sl)]]
    pooled = np.sort(np.hstack([e_pl, e_lp]))
    lo = 95 * (len(pooled) - 1) // 100
    want_sq = np.array([e_pl.max(), e_lp.max(), pooled[lo], pooled[min(lo + 1, len(pooled) - 1)]], F32)
    assert np.array_equal(bits(sq[0].cpu().numpy()), bits(want_sq)), (sq.tolist(), want_sq)
    for k, e in enumerate((e_pl, e_lp)):
        assert _rel(float(sums[0, k]), float(np.sqrt(e.astype(np.float64)).sum())) <= SUM_RTOL
        assert within[0, k].tolist() == [int((e <= tol_sq(t)).sum()) for t in tols]
    assert within[0, :, 2].tolist() == counts[0].tolist() and 0 < int(within[0, 0, 0]) < len(sp)
    assert lesions.tolist() == [[4, 4, 1, 1]]


# ---- 5. empty classes -------------------------------------------------------------------------------------------------------
def test_classes_missing_in_the_prediction_the_truth_and_both(ops):
    classes, tols = ((1,), (2,), (3,)), (1.0, 1000.0)
    pred, truth = blocky(SHAPE, (0, 2), 71), blocky(SHAPE, (0, 1), 72)       # class 0: no prediction, 1: no truth, 2: neither
    per = [(*ref_surface_counts_mm(np.isin(pred, c), np.isin(truth, c), ANISO), lesion_counts(np.isin(pred, c), np.isin(truth, c)),
            ref_within(np.isin(pred, c), np.isin(truth, c), ANISO, tols)) for c in classes]
    counts, sq, sums, within, lesions = check_against(ops, dev(pred), dev(truth), classes, ANISO, per, tols)
    n_l, n_p = int(counts[0, 1]), int(counts[1, 0])
    assert counts.tolist() == [[0, n_l], [n_p, 0], [0, 0]] and n_l > 0 and n_p > 0
    assert not within.any()                              # a +inf distance is never within, whatever the tolerance
    assert not sq.any() and not sums.any()
    assert lesions[0, 0] > 0 and lesions[0].tolist() == [int(lesions[0, 0]), 0, int(lesions[0, 0]), 0]
    assert lesions[1].tolist() == [0, int(lesions[1, 1]), 0, int(lesions[1, 1])] and lesions[2].tolist() == [0] * 4
    nsds = [score.nsd(int(within[c, 0, 1]), int(within[c, 1, 1]), int(counts[c, 0]), int(counts[c, 1])) for c in range(3)]
    assert nsds == [0.0, 0.0, 1.0]


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------
def test_a_workspace_full_of_ones_gives_the_same_bits_twice(ops):
    pred, truth, _ = reference(SHAPE, BRATS, ANISO, (41, 42), TOLS8)
    p, t, lut = dev(pred), dev(truth), Cf.score_class_lut(BRATS)
    first = [x.clone() for x in label_surface_mm(ops, p, t, lut, 3, ANISO, TOLS8)] + [label_lesions(ops, p, t, lut, 3).clone()]
    runs = []
    for _ in range(2):
        ops._ws["surf_mm"].fill_(0xFF)
        ops._ws["cc"].fill_(0xFF)
        runs.append([x.clone() for x in label_surface_mm(ops, p, t, lut, 3, ANISO, TOLS8)] +
                    [label_lesions(ops, p, t, lut, 3).clone()])
    for run in runs:
        for a, b in zip(first, run):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---- 7. argument errors -----------------------------------------------------------------------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_argument_errors_leave_the_outputs_untouched(ops):
    D, H, W, Cc = 5, 6, 7, 2
    ARG, WS = 1, 3
    assert _lib._ERR_NAMES[ARG] == "EFFQ_ERR_ARG" and _lib._ERR_NAMES[WS] == "EFFQ_ERR_WORKSPACE"
    lib, stream = ops.lib, ops.stream
    pred = dev(blocky((D, H, W), (0, 1, 2), 81))
    truth = dev(blocky((D, H, W), (0, 1, 2), 82))
    lut = (C.c_uint16 * 256)(*Cf.score_class_lut(LITS))
    bad_lut = (C.c_uint16 * 256)(*([0, 1, 3] + [0] * 252 + [4]))              # bit 2 with two classes
    counts = torch.full((Cc, 2), 7, dtype=torch.int64, device=DEV)
    sq = torch.full((Cc, 4), 7.0, dtype=torch.float32, device=DEV)
    sums = torch.full((Cc, 2), 7.0, dtype=torch.float64, device=DEV)
    within = torch.full((Cc, 2, 8), -1, dtype=torch.int64, device=DEV)
    les = torch.full((Cc, 4), 7, dtype=torch.int64, device=DEV)
    need = lib.effq_label_surface_mm_ws_bytes(Cc, D, H, W, 8)
    assert need == (lib.effq_surf_mm_ws_bytes(2 * Cc, D, H, W) + 15) // 16 * 16 + 1152
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def surf(tols=(1.0,), ntol=None, pp=_ptr(pred), tp=_ptr(truth), ncls=Cc, dims=(D, H, W), table=lut, wts=(25.0, 0.5, 0.5),
             cp=_ptr(counts), qp=_ptr(sq), sp=_ptr(sums), wi=_ptr(within), wp=_ptr(ws), nbytes=need, tolp=True):
        t = (C.c_float * max(len(tols), 1))(*tols)
        return lib.effq_label_surface_mm(pp, tp, ncls, *dims, table, *wts, t if tolp else None,
                                         len(tols) if ntol is None else ntol, cp, qp, sp, wi, wp, nbytes, stream)
    assert surf(tols=[0.0] * 9) == ARG and surf(ntol=9) == ARG and surf(ntol=-1) == ARG
    assert surf(tols=[-1.0]) == ARG and surf(tols=[float("nan")]) == ARG and surf(tols=[float("inf")]) == ARG
    assert surf(tols=[2.0, 1.0]) == ARG and surf(tols=[1.0, 1.0]) == ARG and surf(tols=[0.0, 1.0, float("nan")]) == ARG
    assert surf(table=bad_lut) == ARG and surf(table=None) == ARG
    for null in ("pp", "tp", "cp", "qp", "sp", "wi", "wp"):
        assert surf(**{null: None}) == ARG, null
    assert surf(tolp=False) == ARG
    assert surf(nbytes=need - 1) == ARG and surf(nbytes=0) == ARG
    assert surf(ncls=0) == ARG and surf(ncls=9) == ARG and surf(dims=(4097, 1, 1)) == ARG and surf(dims=(0, 6, 7)) == ARG
    for k, bad in ((0, 0.0), (1, -0.5), (2, float("nan")), (0, float("inf"))):
        wts = [25.0, 0.5, 0.5]
        wts[k] = bad
        assert surf(wts=wts) == ARG, (k, bad)
    need_cc = lib.effq_cc_ws_bytes(2 * Cc, D, H, W)
    ws_cc = torch.zeros(need_cc, dtype=torch.uint8, device=DEV)

    def lesions(pp=_ptr(pred), tp=_ptr(truth), ncls=Cc, dims=(D, H, W), table=lut, conn=26, cp=_ptr(les), wp=_ptr(ws_cc),
                nbytes=need_cc):
        return lib.effq_label_lesions(pp, tp, ncls, *dims, table, conn, cp, wp, nbytes, stream)
    assert lesions(table=bad_lut) == ARG and lesions(table=None) == ARG and lesions(conn=18) == ARG
    for null in ("pp", "tp", "cp", "wp"):
        assert lesions(**{null: None}) == ARG, null
    assert lesions(ncls=0) == ARG and lesions(ncls=9) == ARG and lesions(dims=(0, 6, 7)) == ARG
    assert lesions(dims=(2048, 1024, 1024)) == ARG and lesions(nbytes=need_cc - 1) == WS
    torch.cuda.synchronize()
    assert (counts == 7).all() and (sq == 7).all() and (sums == 7).all() and (within == -1).all() and (les == 7).all()
    # ntol = 0 with a null within succeeds and leaves a given one alone
    assert surf(tols=(), wi=None, tolp=False) == 0 and surf(tols=()) == 0
    torch.cuda.synchronize()
    assert (within == -1).all() and (counts != 7).any()
    assert surf(tols=(1.0, 2.0)) == 0 and lesions() == 0
    torch.cuda.synchronize()
    flat = within.reshape(-1)
    assert (flat[:Cc * 2 * 2] >= 0).all() and (flat[Cc * 2 * 2:] == -1).all()      # (C, 2, ntol) words and no more
    # the python front names the argument
    p, t, table = pred, truth, Cf.score_class_lut(LITS)
    for call in (lambda **kw: label_lesions(ops, kw.get("p", p), kw.get("t", t), kw.get("lut", table), kw.get("C", 2)),
                 lambda **kw: label_surface_mm(ops, kw.get("p", p), kw.get("t", t), kw.get("lut", table), kw.get("C", 2),
                                               (1, 1, 1))):
        for kw, named in ((dict(p=p.float()), "pred"), (dict(t=t.cpu()), "truth"), (dict(t=t[:, :, :6]), "truth"),
                          (dict(p=p[0]), "pred"), (dict(lut=table[:255]), "lut"), (dict(lut=[4] * 256), "lut"),
                          (dict(C=0), "classes"), (dict(C=9), "classes")):
            with pytest.raises(_lib.EffqError, match=named):
                call(**kw)
    with pytest.raises(_lib.EffqError, match="connectivity"):
        label_lesions(ops, p, t, table, 2, connectivity=18)
    with pytest.raises(_lib.EffqError, match="spacing"):
        label_surface_mm(ops, p, t, table, 2, (1, 0, 1))
    for bad in ((-1,), (2, 1), (float("nan"),), tuple(range(9))):
        with pytest.raises(_lib.EffqError, match="tols"):
            label_surface_mm(ops, p, t, table, 2, (1, 1, 1), bad)
    assert tolerances_sq("t", (0.7421875,)) == [float(tol_sq(0.7421875))]


# ---- 8. the mission on the device -----------------------------------------------------------------------------------------------
def test_mission_writes_the_numbers_of_the_yardsticks(tmp_path, capsys):
    root = str(tmp_path)
    maps = {"a": (blobs(1), blobs(2)), "b": (np.where(blobs(3) == 2, 1, blobs(3)).astype(np.uint8), blobs(4)),
            "c": (blobs(5), blobs(5)), "u": (blobs(6), None)}
    lst = write_pairs(root, maps)
    out = os.path.join(root, "score")
    entrance.main(["score", "--task", "lits", "--src_list", lst, "--pred_dir", os.path.join(root, "pred"), "--out_dir", out,
                   "--score_tol", "3,0.75"])
    said = capsys.readouterr().out
    assert "skipped: u" in said and "3 subjects scored" in said
    tols = (0.75, 3.0)
    rows = list(csv.reader(open(os.path.join(out, "scores.csv"))))
    assert rows[0] == list(score.SCORE_COLUMNS) + ["nsd_0.75mm", "nsd_3mm"] and len(rows) == 1 + 3 * 2
    ml = float(np.prod(FILE_SPACING)) / 1000.0
    k = 1
    for sn in "abc":
        pred, truth = maps[sn]
        for c, labels in enumerate(LITS):
            p, t = np.isin(pred, labels), np.isin(truth, labels)
            tp, fp, fn, tn = int((p & t).sum()), int((p & ~t).sum()), int((~p & t).sum()), int((~p & ~t).sum())
            n_p, n_l = int(ref_surface(p).sum()), int(ref_surface(t).sum())
            w = ref_within(p, t, FILE_SPACING, tols)
            nsds = [score.nsd(w[0][j], w[1][j], n_p, n_l) for j in range(2)]
            want = [sn, str(c), " ".join(str(v) for v in labels)] + [g7(v) for v in f32_ratios(tp, fp, fn, tn)] + \
                [str(v) for v in (tp, fp, fn, tn)] + [g7((tp + fp) * ml), g7((tp + fn) * ml)] + \
                [str(v) for v in lesion_counts(p, t)] + [g7(v) for v in ref_surface_metrics_mm(p, t, FILE_SPACING)] + \
                [g7(v) for v in nsds]
            assert rows[k] == want, (rows[k], want)
            k += 1
    assert rows[5][3] == "1" and rows[5][-2:] == ["1", "1"] and rows[5][17:20] == ["0", "0", "0"]      # c: the map is the truth
    assert rows[4][-2:] == ["0", "0"]                                                                   # b: no tumour predicted
    summ = list(csv.reader(open(os.path.join(out, "summary.csv"))))
    assert summ[0] == list(score.summary_columns(tols)) and [r[2] for r in summ[1:]] == ["3", "3"]
    for c in range(2):
        mine = [r for r in rows[1:] if r[1] == str(c)]
        assert summ[1 + c][-6:-2] == [str(sum(int(r[13 + j]) for r in mine)) for j in range(4)]
