"""--prep_register rigid on the host: the switch, the objective, the transform, and the prep mission on a stand-in."""
import csv
import math
import os

import numpy as np
import pytest
import torch

from efficientq_amd import entrance, prep, register as G
from tests import prep_align_ref as A
from tests import prep_register_ref as R
from tests import test_prep_align_cpu as H
from tests.test_prep_cpu import prep_args, ref_standardise_crop, write_list, write_scan

EYE = np.eye(4)


class RegisterOps(R.RegisterMixin, H.AlignOps):
    """The stand-in for the device with the calls of the registration."""


PREP = ["prep", "--task", "brats", "--src_list", "none.csv", "--data_dir", "o", "--prep_register"]
A_SEG = A.affine((1.0, 1.0, 1.0), (1.0, 0.0, 2.0))          # the label: the reference's grid from its voxel (1, 0, 2) on


@pytest.mark.parametrize("argv, named", [
    (PREP + ["affine", "--prep_align", "t1"], "--prep_register 'affine': rigid"),
    (PREP + ["rigid"], "it needs --prep_align MODALITY"),
    (["ptq", "--task", "brats", "--synthetic", "--prep_register", "rigid"], "ptq mission"),
    (["score", "--task", "lits", "--src_list", "c", "--pred_dir", ".", "--out_dir", "o", "--prep_register", "rigid"],
     "score mission"),
])
def test_the_switch_is_refused_by_name_before_a_file_is_read(argv, named):
    with pytest.raises(SystemExit) as e:
        entrance.main(argv)
    assert "--prep_register" in str(e.value) and named in str(e.value) and not os.path.exists("o")


@pytest.mark.parametrize("hist, want", [
    (np.diag([5, 0, 3, 8]), 2.0), (np.outer([1, 0, 3], [2, 2, 0]), 1.0),      # a bijection of the bins; independent bins
    (np.array([[4, 1, 0], [0, 0, 0], [2, 0, 9]]), None), (np.zeros((4, 4)), 0.0), (np.diag([0, 7, 0, 0]), 0.0)])
def test_nmi_against_the_formula_on_hand_made_histograms_with_empty_rows(hist, want):
    p = hist / max(hist.sum(), 1)
    ent = [-sum(v * math.log(v) for v in q.reshape(-1) if v > 0) for q in (p.sum(1), p.sum(0), p)]
    assert G.nmi(hist) == pytest.approx((ent[0] + ent[1]) / ent[2] if ent[2] > 0 else 0.0, abs=1e-14)
    assert want is None or G.nmi(hist) == pytest.approx(want, abs=1e-14)


def test_rigid_matrix_at_zero_and_a_rotation_about_the_centre_by_hand():
    a_src, n_src, a_ref, n_ref = A.oblique_pair()
    zero = G.rigid_matrix("s", "m", a_src, a_ref, n_ref, (0.0,) * 6)
    assert np.array_equal(zero.view(np.uint64), prep.align_matrix("s", "m", a_src, a_ref).view(np.uint64))
    # a quarter turn about z through the centre (2, 3, 4) of 5 x 7 x 9, then 1 mm along x: (3 - (y - 3), 3 + (x - 2), z)
    m = G.rigid_matrix("s", "m", EYE, EYE, (5, 7, 9), (1.0, 0.0, 0.0, 0.0, 0.0, math.pi / 2))
    assert np.allclose(m, [[0, -1, 0, 6.0], [1, 0, 0, 1.0], [0, 0, 1, 0.0]], atol=1e-15)


def registered_pair(ops, to_device=torch.from_numpy, shape=R.PAIR_SHAPE):
    """(Registered, its greatest corner displacement from the truth in voxels, the levels) of the synthetic pair."""
    true = G.rigid_matrix("s", "mov", EYE, EYE, shape, R.PAIR_THETA)
    fixed, moving = R.synthetic_pair(true, shape)
    ref = G.Reference(ops, "s", "ref", to_device(fixed), EYE)
    got = G.register_rigid(ops, ref, "mov", to_device(moving), EYE)
    n = np.asarray(shape, dtype=np.float64) - 1.0
    corners = np.array([[i, j, k, 1.0] for i in (0, n[0]) for j in (0, n[1]) for k in (0, n[2])])
    err = float(np.linalg.norm(corners @ got.matrix.T - corners @ true.T, axis=1).max())
    print(f"theta {got.theta}, {got.evals} launches, NMI {got.nmi_before!r} -> {got.nmi_after!r}, corner error {err!r}")
    return got, err, [s for s, _ in ref.levels]


def register_subjects(root, names=("r1", "r2")):
    """Two subjects: t1ce the reference, every other modality one moved function of it, the label on a shifted box."""
    os.makedirs(os.path.join(root, "src"), exist_ok=True)
    rows, truth = [], {}
    for i, sn in enumerate(names):
        theta = (0.8, 0.5, -0.6 * (i + 1), 0.0, 0.0, math.radians(1.5 * (i + 1)))
        fixed, moved = R.synthetic_pair(G.rigid_matrix(sn, "m", EYE, EYE, R.PAIR_SHAPE, theta), seed=20 + i)
        seg = (fixed[1:, :, 2:] > 400).astype(np.uint8) + (fixed[1:, :, 2:] > 600)
        truth[sn] = (moved.astype(np.int16), seg.astype(np.uint8))
        row = [sn]
        for name in H.MODS + ("seg",):
            row.append(os.path.join("src", f"{sn}_{name}.nii.gz"))
            scan = fixed.astype(np.int16) if name == "t1ce" else truth[sn][name == "seg"]
            write_scan(os.path.join(root, row[-1]), scan, affine=A_SEG if name == "seg" else EYE)
        rows.append(row)
    return rows, truth


def check_mission(out, truth, aligned_plane, said):
    """The columns after the align columns, a moved plane from the recorded parameters, the label from its header."""
    table = list(csv.DictReader(open(os.path.join(out, prep.PREP_CSV))))
    at = list(table[0]).index("align")
    assert list(table[0])[at:at + 6] == prep.ALIGN_COLUMNS + prep.REGISTER_COLUMNS
    for row in table:
        sn, (moved, seg) = row["subject"], truth[row["subject"]]
        params, nmis, evals = (row[k].split(";") for k in ("register_params", "register_nmi", "register_evals"))
        assert row["register"] == "rigid" and len(params) == len(nmis) == len(evals) == 3 and evals[0].split()[1] == "1"
        assert float(nmis[0].split()[1]) > float(nmis[0].split()[0])
        matrix = G.rigid_matrix(sn, "flair", EYE, EYE, R.PAIR_SHAPE, G.params_theta(params[0]))
        lo, hi = ([int(v) for v in row[k].split()] for k in ("pmin", "pmax"))
        want = aligned_plane(moved.astype(np.float32), matrix, lo, hi, [float(row["flair_mean"])], [float(row["flair_std"])])
        assert np.array_equal(np.load(os.path.join(out, "flair", f"{sn}.npy")), want) and want.any()
        lab, _ = A.align(seg, prep.align_matrix(sn, "seg", A_SEG, EYE), R.PAIR_SHAPE, nearest=True)
        assert np.array_equal(np.load(os.path.join(out, "seg", f"{sn}.npy")), lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
    assert ", registered flair: " in said and "NMI" in said and "the label is never registered" in said


def test_prep_mission_through_the_stand_in(tmp_path, capsys):
    rows, truth = register_subjects(str(tmp_path))
    prep.run(prep_args(src_list=write_list(tmp_path / "cases.csv", rows), data_dir=str(tmp_path / "out"),
                       prep_min_size="8,8,8", prep_align="t1ce", prep_register="rigid"), ops=RegisterOps())
    check_mission(str(tmp_path / "out"), truth, lambda raw, m, lo, hi, mean, std: ref_standardise_crop(
        A.align(raw, m, R.PAIR_SHAPE)[0][None], lo, hi, mean, std, "nonzero")[0], capsys.readouterr().out)
