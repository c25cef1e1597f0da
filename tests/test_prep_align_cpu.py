"""--prep_align on the host: the switch, the matrices, the numpy restatement of effq_prep_align against scipy, and the
prep and predict missions through a stand-in for the device that carries prep_align."""
import csv
import os

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

from efficientq_amd import config as Cf, data as D, entrance, nifti, predict, prep
from tests import prep_align_ref as A
from tests.test_predict_cpu import PredictOps
from tests.test_prep_cpu import NumpyOps, prep_args, write_list, write_scan, written

MODS = D.MODALITIES["brats"]
U24 = 2.0 ** -24


class AlignOps(PredictOps):
    """The stand-in for the device of the prep and predict tests, with prep_align through the restatement."""
    calls = 0

    def prep_align(self, x, matrix, out_shape, nearest=False):
        type(self).calls += 1
        y, inside = A.align(x.numpy(), matrix, out_shape, nearest)
        return torch.from_numpy(y), torch.tensor([inside], dtype=torch.int64)


class FourNet(torch.nn.Module):
    """Four modalities to three classes, voxel by voxel."""

    def forward(self, x):
        s = x.sum(1, keepdim=True) * 0.5
        return torch.cat([0.3 - s * s, s - 0.2, -s - 0.4], 1)


# ---- the switch --------------------------------------------------------------------------------------------------------
def test_parser_yaml_and_the_refusals_of_the_switch(tmp_path):
    a = Cf.build_parser().parse_args(["prep", "--task", "brats", "--prep_align", "t1ce"])
    assert a.prep_align == "t1ce" and prep.parse_options(a, "brats").align == "t1ce"
    assert Cf.build_parser().parse_args(["predict", "--task", "brats"]).prep_align is None
    assert prep.parse_options(Cf.build_parser().parse_args(["prep", "--task", "brats"]), "brats").align is None
    cfg = tmp_path / "p.yaml"
    cfg.write_text("prep_align: t2\n")
    a = Cf.merge_config(str(cfg), a)
    opts = prep.parse_options(a, "brats")
    assert opts.align == "t2" and opts.columns()[-2:] == ["align", "align_inside"] == prep.ALIGN_COLUMNS
    assert prep.PrepOptions._fields[-1] == "align"
    for bad in ("pd", "seg", "", 3):
        a.prep_align = bad
        with pytest.raises(SystemExit) as e:
            prep.parse_options(a, "brats")
        assert str(e.value) == f"--prep_align {bad!r}: one of flair, t1, t1ce, t2"
    # in parse_options' order after --prep_interp
    a.prep_interp = "quintic"
    with pytest.raises(SystemExit) as e:
        prep.parse_options(a, "brats")
    assert "--prep_interp" in str(e.value)
    # cubic and the anti-alias filter keep their meaning: they still need --prep_spacing
    a.prep_interp, a.prep_align = "cubic", "t1"
    with pytest.raises(SystemExit) as e:
        prep.parse_options(a, "brats")
    assert "--prep_spacing" in str(e.value)


def test_score_refuses_the_switch_by_name(tmp_path):
    with pytest.raises(SystemExit) as e:
        entrance.main(["score", "--task", "lits", "--src_list", str(tmp_path / "c.csv"), "--pred_dir", str(tmp_path),
                       "--out_dir", str(tmp_path / "o"), "--prep_align", "ct"])
    assert "--prep_align" in str(e.value) and "score mission" in str(e.value) and not os.path.exists(tmp_path / "o")


# ---- the matrix ----------------------------------------------------------------------------------------------------------
def test_matrix_of_hand_computed_header_pairs():
    scaling = prep.align_matrix("s", "t1", np.diag([2.0, 4.0, 0.5, 1.0]), np.diag([1.0, 1.0, 1.0, 1.0]))
    assert scaling.shape == (3, 4) and scaling.dtype == np.float64
    assert np.array_equal(scaling, [[0.5, 0, 0, 0], [0, 0.25, 0, 0], [0, 0, 2.0, 0]])
    src, ref = np.eye(4), np.eye(4)
    src[:3, 3], ref[:3, 3] = (1.0, 2.0, 3.0), (0.0, 0.5, -1.0)
    assert np.array_equal(prep.align_matrix("s", "t1", src, ref), [[1, 0, 0, -1.0], [0, 1, 0, -1.5], [0, 0, 1, -4.0]])
    # source (i, j, k) lies at world (k, 4 - i, j): i = 4 - y, j = z, k = x
    turned = np.array([[0, 0, 1.0, 0], [-1.0, 0, 0, 4.0], [0, 1.0, 0, 0], [0, 0, 0, 1.0]])
    assert np.array_equal(prep.align_matrix("s", "t2", turned, np.eye(4)), [[0, -1, 0, 4.0], [0, 0, 1, 0], [1, 0, 0, 0]])
    for bad, named in ((np.diag([1.0, 0.0, 1.0, 1.0]), "determinant 0"), (np.diag([1.0, np.nan, 1.0, 1.0]), "not finite"),
                       (np.diag([np.inf, 1.0, 1.0, 1.0]), "not finite")):
        with pytest.raises(SystemExit) as e:
            prep.align_matrix("s9", "t2", bad, np.eye(4))
        assert "subject s9" in str(e.value) and "t2" in str(e.value) and named in str(e.value)
    with pytest.raises(SystemExit) as e:          # a result that is not finite: the reference's own affine
        prep.align_matrix("s9", "t2", np.eye(4), np.diag([1.0, np.inf, 1.0, 1.0]))
    assert "subject s9" in str(e.value) and "t2" in str(e.value) and "not finite" in str(e.value)


# ---- the restatement -------------------------------------------------------------------------------------------------------
def oblique():
    a_src, n_src, a_ref, n_ref = A.oblique_pair()
    return prep.align_matrix("s", "m", a_src, a_ref), n_src, n_ref


def test_restatement_against_scipy_inside_the_field_of_view():
    m, n_src, n_ref = oblique()
    g = np.random.default_rng(0)
    x = g.uniform(-1000.0, 1000.0, n_src).astype(np.float32)
    y, inside = A.align(x, m, n_ref)
    fov = A.field_of_view(A.coordinates(m, n_ref), n_src)
    assert inside == int(fov.sum()) == 2460 and fov.size == 16169
    assert not y[~fov].any() and not np.signbit(y[~fov]).any()
    want = ndi.affine_transform(x.astype(np.float64), m[:, :3], offset=m[:, 3], output_shape=n_ref, order=1, mode="nearest")
    # In units of 2^-24 of max|x|; the inputs are float32 already.  Weights: per axis l1 = float32(c - i0) is off by
    # e1 <= 2^-25 and l0 = 1 - l1 by -e1 + e2 with e2 <= 2^-25, which moves l0 A + l1 B by e1 (B - A) + e2 A <= 1.5 units: 4.5
    # for the three axes.  Operations: the multiplications by lw, the additions along w, and the same for h and for d are
    # six layers, each rounding values whose weighted magnitudes sum to at most max|x| by 2^-25 of them: 3 units.
    # 4.5 + 3 = 7.5 -> 8; scipy's own fp64 arithmetic is eight orders below.
    bound = 8 * U24 * 1000.0
    err = np.abs(y.astype(np.float64) - want)[fov].max()
    print(f"restatement against scipy: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    lab = g.integers(0, 5, n_src).astype(np.uint8)
    got, n = A.align(lab, m, n_ref, nearest=True)
    near = ndi.affine_transform(lab, m[:, :3], offset=m[:, 3], output_shape=n_ref, order=0, mode="nearest")
    assert n == 2460 and np.array_equal(got[fov], near[fov]) and not got[~fov].any()


def test_restatement_identity_and_the_half_voxel_edges():
    g = np.random.default_rng(1)
    x = g.standard_normal((5, 6, 7)).astype(np.float32)
    def shifted(w):         # the source's origin lies -w voxels along w from the reference's
        m = prep.align_matrix("s", "m", A.affine((1.0, 1.0, 1.0), (0.0, 0.0, -w)), np.eye(4))
        assert np.array_equal(m[:, :3], np.eye(3)) and m[:, 3].tolist() == [0.0, 0.0, w]
        return m
    eye = shifted(0.0)
    y, inside = A.align(x, eye, x.shape)
    assert inside == x.size and np.array_equal(y.view(np.uint32), x.view(np.uint32))
    lab = g.integers(0, 255, (5, 6, 7)).astype(np.uint8)
    assert np.array_equal(A.align(lab, eye, lab.shape, nearest=True)[0], lab)
    half = shifted(-0.5)                    # s_w = w - 0.5: -0.5 is inside, and 6 - 0.5 < 7 - 0.5
    y, inside = A.align(x, half, x.shape)
    assert inside == x.size and np.array_equal(y[:, :, 0], x[:, :, 0])            # the edge replicated over the half voxel
    assert np.array_equal(y[:, :, 1:], np.float32(0.5) * x[:, :, :-1] + np.float32(0.5) * x[:, :, 1:])
    assert np.array_equal(A.align(lab, half, lab.shape, nearest=True)[0][:, :, 1:], lab[:, :, 1:])   # floor(w - 0.5 + 0.5)
    past = shifted(-0.5000001)
    y, inside = A.align(x, past, x.shape)
    assert inside == x.size - 5 * 6 and not y[:, :, 0].any() and y[:, :, 1:].all()
    up = shifted(0.5)                       # s_w = w + 0.5: the last column sits at 6.5 = n - 0.5, outside (`<`)
    y, inside = A.align(x, up, x.shape)
    assert inside == x.size - 5 * 6 and not y[:, :, -1].any()
    # one source voxel: the nearest index stays 0 although 0.5 - 2^-54 + 0.5 rounds to 1.0 in fp64
    one = np.array([[7]], dtype=np.uint8).reshape(1, 1, 1)
    edge = np.zeros((3, 4))
    edge[:, 3] = np.nextafter(0.5, 0.0)
    assert A.align(one, edge, (1, 1, 1), nearest=True) == (one, 1)


# ---- one subject on four grids --------------------------------------------------------------------------------------------
GRID = (20, 24, 28)                                          # flair's
A_FLAIR = A.affine((1.0, 1.0, 1.0), (-10.0, -12.0, 3.0))
A_T1 = A.affine((2.0, 2.0, 2.0), (-9.0, -12.5, 4.0))          # 2 x coarser, shifted: 10 x 12 x 14 voxels
A_T1CE = A.affine((1.0, 1.0, 1.0), (-9.0, -12.0, 5.0))       # flair's grid from its voxel (1, 0, 2) on: 18 x 24 x 25
# t2 (k, i, j'): array axis 0 is flair's axis 2, axis 1 flair's axis 0, axis 2 flair's axis 1 reversed
A_T2 = A_FLAIR @ np.array([[0, 1.0, 0, 0], [0, 0, -1.0, 23.0], [1.0, 0, 0, 0], [0, 0, 0, 1.0]])


def align_subject(root, sn="a1", aligned=False):
    """One subject under <root>/src: t1 on a 2 x coarser, shifted grid, t2 with permuted axes, t1ce and the label on a
    shifted box of flair's grid.  With `aligned` every scan lies on flair's grid instead (the same seeds).  Returns the
    row of a --src_list and {name: (array, affine)}."""
    g = np.random.default_rng(11)
    os.makedirs(os.path.join(root, "src"), exist_ok=True)

    def body(shape, margin, scale):
        v = np.zeros(shape, dtype=np.int16)
        inner = tuple(slice(m, n - m) for n, m in zip(shape, margin))
        v[inner] = g.integers(200, 1200, size=v[inner].shape) * scale
        return v
    scans = {"flair": (body(GRID, (2, 3, 4), 1), A_FLAIR), "t1": (body((10, 12, 14), (1, 2, 2), 2), A_T1),
             "t1ce": (body((18, 24, 25), (2, 3, 3), 3), A_T1CE), "t2": (body((28, 20, 24), (4, 2, 3), 4), A_T2)}
    seg = np.zeros((18, 24, 25), dtype=np.uint8)
    seg[3:-3, 4:-4, 4:-4] = g.integers(0, 4, size=seg[3:-3, 4:-4, 4:-4].shape)
    scans["seg"] = (seg, A_T1CE)
    if aligned:
        scans = {k: (g.permutation(body(GRID, (2, 3, 4), 1).ravel()).reshape(GRID) if k != "seg" else
                     np.pad(seg, ((1, 1), (0, 0), (2, 1))), A_FLAIR) for k in scans}
    row = [sn]
    for name in MODS + ("seg",):
        row.append(os.path.join("src", f"{sn}_{name}.nii.gz"))
        write_scan(os.path.join(root, row[-1]), scans[name][0], affine=scans[name][1])
    return row, scans


def on_grid_of(scans, ref):
    """Every scan of align_subject on the grid of `ref` by the restatement: ({name: array}, {name: inside or None})."""
    a_ref, shape = scans[ref][1], scans[ref][0].shape
    out, inside = {}, {}
    for name, (v, aff) in scans.items():
        if np.array_equal(aff, a_ref) and v.shape == shape:
            out[name], inside[name] = (v if name == "seg" else v.astype(np.float32)), None
        else:
            out[name], inside[name] = A.align(v if name == "seg" else v.astype(np.float32),
                                              prep.align_matrix("a1", name, aff, a_ref), shape, nearest=name == "seg")
    return out, inside


def files_equal(one, two, but=()):
    assert [f for f in written(one)] == [f for f in written(two)]
    for f in written(one):
        if f not in but:
            assert open(os.path.join(one, f), "rb").read() == open(os.path.join(two, f), "rb").read(), f


@pytest.mark.parametrize("ref", ["flair", "t1ce"])
def test_prep_aligns_the_subject_onto_the_reference(tmp_path, ref, capsys):
    root, out, flat = str(tmp_path), str(tmp_path / "out"), str(tmp_path / "flat")
    row, scans = align_subject(root)
    lst = write_list(tmp_path / "cases.csv", [row])
    AlignOps.calls = 0
    prep.run(prep_args(src_list=lst, data_dir=out, prep_min_size="8,8,8", prep_align=ref), ops=AlignOps())
    said = capsys.readouterr().out
    want, inside = on_grid_of(scans, ref)
    moved = [n for n in MODS + ("seg",) if inside[n] is not None]
    assert moved == {"flair": ["t1", "t1ce", "t2", "seg"], "t1ce": ["flair", "t1", "t2"]}[ref] and AlignOps.calls == len(moved)
    shape = scans[ref][0].shape
    full = int(np.prod(shape))
    # t2 covers flair's grid exactly, and so t1ce's box of it; t1 does not reach every edge of either
    counts = [full if inside[n] is None else inside[n] for n in MODS + ("seg",)]
    assert all(0 < c <= full for c in counts) and inside["t2"] == full and inside["t1"] < full
    # the same arrays, already on the reference's grid, through the run without the switch: the files are the same
    os.makedirs(os.path.join(flat, "src"))
    cells = [row[0]]
    for name in MODS + ("seg",):
        cells.append(os.path.join("src", f"f_{name}.nii.gz"))
        write_scan(os.path.join(flat, cells[-1]), want[name], affine=scans[ref][1])
    prep.run(prep_args(src_list=write_list(os.path.join(flat, "cases.csv"), [cells]), data_dir=os.path.join(flat, "out"),
                       prep_min_size="8,8,8"), ops=NumpyOps())
    files_equal(out, os.path.join(flat, "out"), but=(prep.PREP_CSV, D.SN_FN_FILE))
    assert np.load(os.path.join(out, "t1", "a1.npy")).any() and np.load(os.path.join(out, "seg", "a1.npy")).any()
    # the reference's own scan is the subject's source image
    assert open(os.path.join(out, D.SN_FN_FILE)).read() == f"a1,{os.path.join(root, 'src', f'a1_{ref}.nii.gz')}\n"
    table = list(csv.reader(open(os.path.join(out, prep.PREP_CSV))))
    base = list(csv.reader(open(os.path.join(flat, "out", prep.PREP_CSV))))
    assert table[0] == base[0] + ["align", "align_inside"] and table[1][:-2] == base[1]
    assert table[1][-2:] == [ref, " ".join(str(c) for c in counts)]
    assert table[1][1] == " ".join(str(n) for n in shape)
    line = f", aligned to {ref}: " + ", ".join(f"{n} {c / full:.2f}" for n, c in zip(MODS + ("seg",), counts) if n in moved)
    assert line in said and "1.00" in line


def test_prep_refusals_under_the_switch_and_without_it(tmp_path):
    root, out = str(tmp_path), str(tmp_path / "out")
    row, scans = align_subject(root)
    lst = write_list(tmp_path / "cases.csv", [row])

    def refused(named, by_headers=True, **over):
        with pytest.raises(SystemExit) as e:
            prep.run(prep_args(src_list=lst, data_dir=out, prep_min_size="8,8,8", **over), ops=AlignOps())
        assert all(n in str(e.value) for n in named), str(e.value)
        assert not os.path.exists(out) if by_headers else written(out) == []      # what the voxels decide: at the subject
    # without the switch: today's words, for the first header that differs
    refused(["subject a1: t1 has shape (10, 12, 14), the first modality (20, 24, 28)"])
    refused(["--prep_align 'pd': one of flair, t1, t1ce, t2"], prep_align="pd")
    t2 = os.path.join(root, row[4])
    far = A_T2.copy()
    far[:3, 3] += 500.0                         # half a metre away: no voxel of the grid lies inside t2
    write_scan(t2, scans["t2"][0], affine=far)
    refused(["subject a1", "t2", "no voxel of the reference grid lies inside it; do the headers share a world?"],
            by_headers=False, prep_align="flair")
    os.rmdir(out)
    flat = A_T2.copy()
    flat[:3, 1] = 0.0
    write_scan(t2, scans["t2"][0], affine=flat)
    refused(["subject a1", "t2", "determinant 0"], prep_align="flair")
    nan = A_T2.copy()
    nan[1, 3] = np.nan
    write_scan(t2, scans["t2"][0], affine=nan)
    refused(["subject a1", "t2", "not finite"], prep_align="flair")
    # an array that does not hold what its own header says is still refused, against its own header
    write_scan(t2, scans["t2"][0], affine=A_T2)
    plan = prep.parse_options(prep_args(prep_min_size="8,8,8", prep_align="flair"), "brats").plan(
        prep.read_src_list(lst, "brats")[0], MODS)
    assert plan.ref == "flair" and sorted(plan.align) == ["seg", "t1", "t1ce", "t2"] and plan.shapes["t1"] == (10, 12, 14)
    imgs = {m: scans[m][0].astype(np.float32) for m in MODS}
    imgs["t1"] = imgs["t1"][:, :, :-1]
    with pytest.raises(SystemExit) as e:
        prep.process_subject(AlignOps(), plan, imgs, scans["seg"][0], MODS,
                             prep.parse_options(prep_args(prep_min_size="8,8,8", prep_align="flair"), "brats"))
    assert "t1 holds an array of shape (10, 12, 13), its header says (10, 12, 14)" in str(e.value)


def test_aligned_data_with_the_switch_gives_the_files_of_the_run_without_it(tmp_path):
    root = str(tmp_path)
    row, _ = align_subject(root, aligned=True)
    lst = write_list(tmp_path / "cases.csv", [row])
    AlignOps.calls = 0
    prep.run(prep_args(src_list=lst, data_dir=os.path.join(root, "with"), prep_min_size="8,8,8", prep_align="flair"),
             ops=AlignOps())
    prep.run(prep_args(src_list=lst, data_dir=os.path.join(root, "without"), prep_min_size="8,8,8"), ops=NumpyOps())
    assert AlignOps.calls == 0                  # no launch
    files_equal(os.path.join(root, "with"), os.path.join(root, "without"), but=(prep.PREP_CSV,))
    table = list(csv.reader(open(os.path.join(root, "with", prep.PREP_CSV))))
    base = list(csv.reader(open(os.path.join(root, "without", prep.PREP_CSV))))
    full = str(int(np.prod(GRID)))
    assert table[0] == base[0] + ["align", "align_inside"] and table[1] == base[1] + ["flair", " ".join([full] * 5)]


# ---- predict -------------------------------------------------------------------------------------------------------------
def predict_args(**over):
    a = Cf.build_parser().parse_args(["predict", "--task", "brats"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("ref", ["flair", "t1ce"])
def test_predict_writes_the_map_on_the_reference_grid(tmp_path, ref):
    root, out, flat = str(tmp_path), str(tmp_path / "seg"), str(tmp_path / "flat")
    row, scans = align_subject(root)
    lst = write_list(tmp_path / "cases.csv", [row])
    model = FourNet()
    kw = dict(out_dir=out, patch_size="8,8,8", prep_min_size="8,8,8")
    with pytest.raises(SystemExit) as e:
        predict.run(predict_args(src_list=lst, **kw), ops=AlignOps(), model=model, window_batch=3)
    assert "subject a1: t1 has shape (10, 12, 14), the first modality (20, 24, 28)" in str(e.value)
    assert not os.path.exists(out)
    rows = predict.run(predict_args(src_list=lst, prep_align=ref, **kw), ops=AlignOps(), model=model, window_batch=3)
    want, inside = on_grid_of({k: v for k, v in scans.items() if k != "seg"}, ref)
    shape = scans[ref][0].shape
    got, h = nifti.read_nifti(os.path.join(out, "a1.nii.gz"))
    assert got.shape == shape and got.dtype == np.uint8 and np.allclose(h["affine"], scans[ref][1])
    assert len(np.unique(got)) > 1
    # the same map as from scans that lie on the reference's grid already
    os.makedirs(os.path.join(flat, "src"))
    cells = [row[0]]
    for name in MODS:
        cells.append(os.path.join("src", f"f_{name}.nii.gz"))
        write_scan(os.path.join(flat, cells[-1]), want[name], affine=scans[ref][1])
    base = predict.run(predict_args(src_list=write_list(os.path.join(flat, "cases.csv"), [cells], head=("subject",) + MODS),
                                    out_dir=os.path.join(flat, "seg"), patch_size="8,8,8", prep_min_size="8,8,8"),
                       ops=AlignOps(), model=model, window_batch=3)
    assert np.array_equal(got, nifti.read_nifti(os.path.join(flat, "seg", "a1.nii.gz"))[0])
    full = int(np.prod(shape))
    counts = " ".join(str(full if inside[n] is None else inside[n]) for n in MODS)
    assert rows[0]["align"] == ref and rows[0]["align_inside"] == counts
    assert {k: v for k, v in rows[0].items() if k not in ("align", "align_inside")} == base[0]
    table = list(csv.reader(open(os.path.join(out, predict.PREDICT_CSV))))
    assert table[0] == predict.CSV_HEADER + ["align", "align_inside"] and table[1][-2:] == [ref, counts]
    assert table[1][1] == " ".join(str(n) for n in shape)
