"""--prep_orient, host side (no GPU): the orientation a scan's affine gives it and what is refused, the plan, its inverse
and its affine over all 48 orientations, the parser, the C-ABI rows of effq_prep_reorient, and the `prep` and `predict`
missions driven through numpy stand-ins whose prep_reorient is numpy.flip(numpy.transpose(...)) (ref_reorient below, also
what the GPU tests compare the kernels with)."""
import csv
import itertools
import os
import pickle
import re

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, data as D, nifti, predict, prep
from tests.test_post_cpu import PostOps
from tests.test_predict_cpu import PointNet, ct_like, predict_args
from tests.test_prep_cpu import NumpyOps, brats_like, prep_args, write_list, write_scan, written

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERMS = list(itertools.permutations(range(3)))
FLIPS = list(itertools.product((False, True), repeat=3))
# the issue's tolerances of a NIfTI header's float32 affine: relative on the 3 x 3 part, millimetres on the translation
AFFINE_RTOL, AFFINE_TRANSLATION_MM = 1e-6, prep.AFFINE_TRANSLATION_TOL_MM
# the canonical scan is RAS, anisotropic and off-centre
CANON = np.array([[1.5, 0, 0, -3.0], [0, 1.0, 0, 4.0], [0, 0, 2.0, 5.0], [0, 0, 0, 1.0]])
# the stored variants: (src_axis, flip) applied to the canonical arrays: every permutation, every axis flipped, the identity
VARIANTS = [((0, 1, 2), (False, False, False)), ((0, 2, 1), (True, False, False)), ((1, 0, 2), (False, True, False)),
            ((1, 2, 0), (False, False, True)), ((2, 0, 1), (True, True, False)), ((2, 1, 0), (True, True, True)),
            ((0, 1, 2), (True, False, True))]


def ref_reorient(x, src_axis, flip):
    """Output axis p of the last three axes is source axis src_axis[p], reversed iff flip[p]; leading axes stay."""
    lead = x.ndim - 3
    y = np.transpose(x, tuple(range(lead)) + tuple(lead + a for a in src_axis))
    return np.ascontiguousarray(np.flip(y, tuple(lead + p for p in range(3) if flip[p])))


def variant_affine(affine, src_axis, flip, shape):
    """The affine of ref_reorient(x, src_axis, flip) for x of `shape` with `affine`, composed by hand: stored index n sits
    at canonical index s, s[src_axis[p]] = shape[src_axis[p]] - 1 - n[p] if flip[p] else n[p]."""
    out = np.zeros((4, 4))
    out[:, 3] = affine[:, 3]
    for p, (a, f) in enumerate(zip(src_axis, flip)):
        out[:, p] = -affine[:, a] if f else affine[:, a]
        if f:
            out[:, 3] = out[:, 3] + affine[:, a] * (shape[a] - 1)
    return out


def variant_code(src_axis, flip, code="RAS"):
    other = {"R": "L", "L": "R", "A": "P", "P": "A", "S": "I", "I": "S"}
    return "".join(other[code[a]] if f else code[a] for a, f in zip(src_axis, flip))


class OrientNumpyOps(NumpyOps):
    def __init__(self):
        self.reoriented = []

    def prep_reorient(self, x, src_axis, flip):
        self.reoriented.append((tuple(x.shape), str(x.dtype), tuple(src_axis), tuple(bool(f) for f in flip)))
        return torch.from_numpy(ref_reorient(x.numpy(), src_axis, flip))


class OrientPredictOps(PostOps):
    def __init__(self):
        super().__init__()
        self.reoriented = []

    prep_reorient = OrientNumpyOps.prep_reorient


# ---- orientation from affines ------------------------------------------------------------------------------------------
def _code(affine):
    return prep.orient_code(*prep.scan_orientation(affine))


def test_orientation_of_plain_permuted_and_oblique_affines():
    assert prep.scan_orientation(np.diag([1.0, 1, 1, 1])) == ((0, 1, 2), (1, 1, 1)) and _code(np.eye(4)) == "RAS"
    assert prep.scan_orientation(np.diag([-1.0, -1, 1, 1])) == ((0, 1, 2), (-1, -1, 1))
    assert _code(np.diag([-1.0, -1, 1, 1])) == "LPS"
    # the slice axis first, pixdim 0.7, 0.7, 5: array axis 0 runs towards I, axis 1 towards R, axis 2 towards P
    aff = np.array([[0, 0.7, 0, 1.0], [0, 0, -0.7, 2.0], [-5.0, 0, 0, 3.0], [0, 0, 0, 1.0]])
    assert prep.scan_orientation(aff) == ((2, 0, 1), (-1, 1, -1)) and _code(aff) == "IRP"
    c, s = np.cos(np.deg2rad(20.0)), np.sin(np.deg2rad(20.0))
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    aff = np.eye(4)
    aff[:3, :3] = rot @ np.diag([-0.8, 0.8, 2.5])
    assert _code(aff) == "LAS"                                   # 20 degrees about z: the nearest axes
    assert _code(CANON) == "RAS" and prep.orient_code((2, 0, 1), (1, -1, 1)) == "SLA"


def test_affines_without_an_orientation_are_refused_and_the_plan_names_the_subject(tmp_path):
    h = np.sqrt(0.5)
    turned = np.array([[h, -h, 0, 0], [h, h, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])       # exactly 45 degrees
    zero, nan, shear = np.eye(4), np.eye(4), np.eye(4)
    zero[:3, 1] = 0.0
    nan[1, 2] = np.nan
    shear[:3, 1] = (0.9, 0.5, 0.0)                              # axes 0 and 1 both nearest to x
    cases = [(turned, "45 degrees"), (zero, "length 0"), (nan, "length nan"), (shear, "same world axis")]
    for aff, cause in cases:
        with pytest.raises(prep.PrepError, match=cause):
            prep.scan_orientation(aff)
    vol = ct_like(1)[0]
    for i, (aff, cause) in enumerate(cases):
        path = write_scan(tmp_path / f"s{i}.nii.gz", vol, affine=aff)
        entry = {"subject": f"case{i}", "images": {"ct": path}, "seg": None}
        with pytest.raises(SystemExit) as e:
            prep._Plan(entry, ("ct",), None, (8, 8, 8), "RAS")
        assert f"subject case{i}" in str(e.value) and cause in str(e.value) and "--prep_orient" in str(e.value)
        plan = prep._Plan(entry, ("ct",), None, (8, 8, 8))       # without the switch the affine is not judged
        assert plan.orient is None and plan.orient_code is None and plan.oriented_shape == plan.source_shape


# ---- the plan and its affine ---------------------------------------------------------------------------------------------
def test_plan_affine_and_inverse_over_all_48_orientations():
    shape = (3, 4, 5)
    x = np.arange(60).reshape(shape)
    seen = set()
    for perm in PERMS:
        for fl in FLIPS:
            # a scan stored as ref_reorient(canonical, perm, fl) has this affine; ask for RAS and for its own code
            aff = variant_affine(CANON, perm, fl, shape)
            sshape = tuple(shape[a] for a in perm)
            world, sign = prep.scan_orientation(aff)
            own = prep.orient_code(world, sign)
            assert own == variant_code(perm, fl)
            seen.add(own)
            assert prep.orient_plan(world, sign, own, sshape) == ((0, 1, 2), (False, False, False), sshape)
            src, flip, out = prep.orient_plan(world, sign, "RAS", sshape)
            assert out == shape and prep.orient_is_identity(src, flip) == (own == "RAS")
            stored = ref_reorient(x, perm, fl)
            back = ref_reorient(stored, src, flip)
            assert np.array_equal(back, x)                       # RAS again: the canonical array itself
            got = prep.orient_affine(aff, src, flip, sshape)
            assert np.allclose(got, CANON, rtol=0, atol=1e-9)
            for n in itertools.product(*(range(k) for k in out)):
                s = [0, 0, 0]
                for p in range(3):
                    s[src[p]] = sshape[src[p]] - 1 - n[p] if flip[p] else n[p]
                assert back[n] == stored[tuple(s)]
                assert np.abs(got @ [*n, 1] - aff @ [*s, 1]).max() <= 1e-9
            inv = prep.orient_inverse(src, flip)
            assert np.array_equal(ref_reorient(back, *inv), stored)
            assert np.array_equal(ref_reorient(ref_reorient(x, src, flip), *prep.orient_inverse(src, flip)), x)
    assert len(seen) == 48


# ---- the parser and the symbols --------------------------------------------------------------------------------------------
def test_parser_yaml_and_the_codes_that_are_refused_by_name(tmp_path):
    a = Cf.build_parser().parse_args(["prep", "--task", "brats", "--prep_orient", "ras"])
    assert a.prep_orient == "ras" and prep.parse_orient(a.prep_orient) == "RAS" and prep.parse_orient(None) is None
    assert prep.parse_orient("Sar") == "SAR" and prep.parse_orient("LPS") == "LPS"
    assert Cf.build_parser().parse_args(["ptq"]).prep_orient is None
    cfg = tmp_path / "p.yaml"
    cfg.write_text("prep_orient: LPS\n")
    assert Cf.merge_config(str(cfg), a).prep_orient == "LPS"
    rows, _ = _write_variant(str(tmp_path), "a", 1, VARIANTS[0])
    lst = write_list(tmp_path / "cases.csv", [rows])
    for mission, kw in ((prep, dict(data_dir=str(tmp_path / "out"))), (predict, dict(out_dir=str(tmp_path / "out")))):
        for bad in ("RAX", "RRS", "RA", "RLS", "RASS", ""):
            make = prep_args if mission is prep else predict_args
            args = make(src_list=lst, prep_min_size="8,8,8", patch_size="8,8,8", prep_orient=bad, **kw)
            with pytest.raises(SystemExit) as e:
                mission.run(args, ops=OrientNumpyOps(), **({"model": PointNet()} if mission is predict else {}))
            assert isinstance(e.value, prep.PrepError) and f"--prep_orient {bad!r}" in str(e.value)
            assert not os.path.exists(tmp_path / "out")


def test_reorient_symbols_in_header_and_lib_have_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = dict(re.findall(r"\bint (effq_prep_reorient\w*)\s*\((.*?)\)\s*;", code, flags=re.S))
    assert sorted(found) == ["effq_prep_reorient", "effq_prep_reorient_plan"]

    def ctype(decl):
        return _lib._P if "*" in decl else {"int": _lib._I}[decl.split()[0]]
    for name, args in found.items():
        res, got = _lib.SIGNATURES[name]
        assert res == _lib._I and got == [ctype(a.strip()) for a in args.split(",")], name
    assert len(_lib.SIGNATURES["effq_prep_reorient"][1]) == 10 and len(_lib.SIGNATURES["effq_prep_reorient_plan"][1]) == 4
    assert "reorient.hip" in open(os.path.join(ROOT, "efficientq_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "efficientq_amd", "csrc", "reorient.hip")).read()
    body = re.sub(r"//.*", "", src)
    assert not re.search(r"atomic\w*\s*\(", body) and "asm" not in body      # no atomics, no inline assembly


# ---- the prep mission ------------------------------------------------------------------------------------------------------
def _write_variant(root, sn, seed, variant, with_seg=True):
    """The canonical brats-like subject of `seed` stored as `variant`; returns the row of a --src_list."""
    vols, seg, _ = brats_like(seed)
    src, flip = variant
    aff = variant_affine(CANON, src, flip, vols[0].shape)
    os.makedirs(os.path.join(root, "src"), exist_ok=True)
    cells = [sn]
    for c, m in enumerate(D.MODALITIES["brats"]):
        cells.append(os.path.join("src", f"{sn}_{m}.nii.gz"))
        write_scan(os.path.join(root, cells[-1]), ref_reorient(vols[c], src, flip), affine=aff)
    if with_seg:
        cells.append(os.path.join("src", f"{sn}_seg.nii.gz"))
        write_scan(os.path.join(root, cells[-1]), ref_reorient(seg, src, flip), affine=aff)
    return cells, aff


def _affine_close(got, want):
    scale = np.abs(want[:3, :3]).max()
    return np.abs(got[:3, :3] - want[:3, :3]).max() <= AFFINE_RTOL * scale and \
        np.abs(got[:3, 3] - want[:3, 3]).max() <= AFFINE_TRANSLATION_MM


@pytest.mark.parametrize("spacing", [None, "2,1.5,2"])
def test_prep_of_every_stored_variant_equals_prep_of_the_canonical_scan(tmp_path, spacing, capsys):
    root = str(tmp_path)
    names = [f"v{i}" for i in range(len(VARIANTS))]
    rows = [_write_variant(root, sn, 11, v)[0] for sn, v in zip(names, VARIANTS)]
    lst = write_list(tmp_path / "cases.csv", rows)
    canon = write_list(tmp_path / "canon.csv", [rows[0]])                    # v0 is the canonical scan itself
    mods = D.MODALITIES["brats"]
    kw = dict(prep_min_size="6,6,6", prep_spacing=spacing)
    ops0 = OrientNumpyOps()
    prep.run(prep_args(src_list=canon, data_dir=os.path.join(root, "plain"), **kw), ops=ops0)
    assert ops0.reoriented == []
    table0 = list(csv.reader(open(os.path.join(root, "plain", prep.PREP_CSV))))
    assert table0[0] == prep.prep_csv_header(mods)                           # without the switch: exactly the old header
    assert os.path.exists(os.path.join(root, "plain", "grid")) == (spacing is not None)
    capsys.readouterr()
    ops = OrientNumpyOps()
    out = os.path.join(root, "out")
    prep.run(prep_args(src_list=lst, data_dir=out, prep_orient="ras", **kw), ops=ops)
    said = capsys.readouterr().out
    # the identity plan launches nothing; every other variant turns its four modalities and its label
    want_calls = []
    for src, flip in VARIANTS[1:]:
        sshape = tuple((20, 24, 28)[a] for a in src)
        plan = prep.orient_plan(*prep.scan_orientation(variant_affine(CANON, src, flip, (20, 24, 28))), "RAS", sshape)[:2]
        want_calls += [((4,) + sshape, "torch.float32") + plan, ((1,) + sshape, "torch.uint8") + plan]
    assert ops.reoriented == want_calls
    info0 = pickle.load(open(os.path.join(root, "plain", D.RESTORE_FILE), "rb"))["v0"]
    info = pickle.load(open(os.path.join(out, D.RESTORE_FILE), "rb"))
    table = list(csv.reader(open(os.path.join(out, prep.PREP_CSV))))
    assert table[0] == prep.prep_csv_header(mods) + ["source_orient", "orient"] == table0[0] + prep.ORIENT_COLUMNS
    lines = open(os.path.join(out, D.SN_FN_FILE)).read().splitlines()
    grid_shape = (20, 24, 28) if spacing is None else (15, 16, 28)
    want_affine = CANON if spacing is None else prep.resample_affine(CANON, (2 / 1.5, 1.5, 1.0))
    for i, (sn, (src, flip)) in enumerate(zip(names, VARIANTS)):
        for m in mods + ("seg",):
            a, b = (open(os.path.join(d, m, f"{n}.npy"), "rb").read()
                    for d, n in ((out, sn), (os.path.join(root, "plain"), "v0")))
            assert a == b and len(a) > 128, (sn, m)
        assert info[sn] == info0 and info[sn]["shape"] == grid_shape
        assert lines[i] == f"{sn},grid/{sn}.nii.gz"                        # also for the identity: one data set is uniform
        g = nifti.read_geometry(os.path.join(out, "grid", f"{sn}.nii.gz"))
        assert g["shape"] == grid_shape and _affine_close(np.asarray(g["affine"], dtype=np.float64), want_affine), sn
        union = nifti.read_nifti(os.path.join(out, "grid", f"{sn}.nii.gz"))[0]
        first = nifti.read_nifti(os.path.join(out, "grid", "v0.nii.gz"))[0]
        assert union.dtype == np.uint8 and np.array_equal(union, first) and 0 < union.sum() < union.size
        row = dict(zip(table[0], table[i + 1]))
        assert row["source_orient"] == variant_code(src, flip) and row["orient"] == "RAS"
        assert row["source_shape"] == prep._fmt(tuple((20, 24, 28)[a] for a in src))         # the scan's own
        assert row["source_spacing"] == prep._fmt(tuple((1.5, 1.0, 2.0)[a] for a in src))
        assert row["grid_shape"] == prep._fmt(grid_shape) and table[i + 1][:-2][3:] == table0[1][3:]
        assert (f"({variant_code(src, flip)} -> RAS)" in said) == (i > 0)
    # the readers of the ptq mission take the oriented geometry from the grid image
    geo = D.read_source_geometry(out, names, "npy", "flair")
    assert all(g["source_shape"] == grid_shape for g in geo)
    assert geo[3]["spacing"] == pytest.approx((1.5, 1.0, 2.0) if spacing is None else (2.0, 1.5, 2.0), rel=1e-6)


def test_min_size_and_spacing_refer_to_the_oriented_axes(tmp_path):
    root = str(tmp_path)
    row, _ = _write_variant(root, "a", 5, VARIANTS[3])                      # stored 24 x 28 x 20, oriented 20 x 24 x 28
    lst = write_list(tmp_path / "cases.csv", [row])
    out = os.path.join(root, "out")
    with pytest.raises(SystemExit) as e:                                    # fits the stored axes, not the oriented ones
        prep.run(prep_args(src_list=lst, data_dir=out, prep_orient="RAS", prep_min_size="24,8,8"), ops=OrientNumpyOps())
    assert "subject a" in str(e.value) and "(20, 24, 28)" in str(e.value) and not os.path.exists(out)
    prep.run(prep_args(src_list=lst, data_dir=out, prep_orient="RAS", prep_min_size="20,24,28"), ops=OrientNumpyOps())
    assert np.load(os.path.join(out, "flair", "a.npy")).shape == (20, 24, 28)
    plan = prep._Plan(prep.read_src_list(lst, "brats")[0], D.MODALITIES["brats"], (3.0, 2.0, 1.0), (1, 1, 1), "SAR")
    assert plan.orient_code == "ASL" and plan.orient == ((1, 0, 2), (False, False, True))
    assert plan.source_shape == (24, 28, 20) and plan.source_spacing == pytest.approx((1.0, 2.0, 1.5))
    assert plan.oriented_shape == (28, 24, 20) and plan.oriented_spacing == pytest.approx((2.0, 1.0, 1.5))
    assert plan.factors == pytest.approx((1.5, 2.0, 1 / 1.5)) and plan.grid_shape == (19, 12, 30)
    assert np.allclose(plan.grid_affine, prep.resample_affine(plan.oriented_affine, plan.factors))


# ---- the predict mission ---------------------------------------------------------------------------------------------------
def _write_ct_variants(root, seed):
    vol, _ = ct_like(seed)
    os.makedirs(os.path.join(root, "src"), exist_ok=True)
    affs = []
    with open(os.path.join(root, "cases.csv"), "w") as f:
        f.write("subject,ct\n")
        for i, (src, flip) in enumerate(VARIANTS):
            affs.append(variant_affine(CANON, src, flip, vol.shape))
            write_scan(os.path.join(root, "src", f"v{i}.nii.gz"), ref_reorient(vol, src, flip), affine=affs[-1])
            f.write(f"v{i},src/v{i}.nii.gz\n")
    with open(os.path.join(root, "canon.csv"), "w") as f:
        f.write("subject,ct\nv0,src/v0.nii.gz\n")
    return os.path.join(root, "cases.csv"), os.path.join(root, "canon.csv"), affs


@pytest.mark.parametrize("post", [None, "1:largest"])
def test_predict_of_every_stored_variant_is_the_transformed_map_of_the_canonical_scan(tmp_path, post):
    root = str(tmp_path)
    lst, canon, affs = _write_ct_variants(root, 3)
    extra = ["--post", post] if post else []
    kw = dict(patch_size="8,8,8", prep_mask="nonzero")
    plain = os.path.join(root, "plain")
    ops0 = OrientPredictOps()
    predict.run(predict_args(*extra, src_list=canon, out_dir=plain, **kw), ops=ops0, model=PointNet(), window_batch=3)
    assert ops0.reoriented == []
    head0 = next(csv.reader(open(os.path.join(plain, predict.PREDICT_CSV))))
    assert head0 == predict.CSV_HEADER + (predict.CSV_POST_COLUMNS if post else [])
    want, _ = nifti.read_nifti(os.path.join(plain, "v0.nii.gz"))
    assert len(np.unique(want)) == 3
    out = os.path.join(root, "seg")
    ops = OrientPredictOps()
    rows = predict.run(predict_args("--blend", "gauss", *extra, src_list=lst, out_dir=out, prep_orient="RAS", **kw), ops=ops,
                       model=PointNet(), window_batch=3)
    assert written(out) == ["predict.csv"] + [f"v{i}.nii.gz" for i in range(len(VARIANTS))]
    table = list(csv.reader(open(os.path.join(out, predict.PREDICT_CSV))))
    assert table[0] == predict.CSV_HEADER + ["source_orient", "orient", "blend", "tta_mirror"] + \
        (["post", "post_changed"] if post else [])
    # per turned variant: the image in, the uint8 map on the oriented grid back out with the inverse plan
    assert len(ops.reoriented) == 2 * (len(VARIANTS) - 1)
    for i, (src, flip) in enumerate(VARIANTS):
        got, h = nifti.read_nifti(os.path.join(out, f"v{i}.nii.gz"))
        scan = nifti.read_geometry(os.path.join(root, "src", f"v{i}.nii.gz"))
        assert got.dtype == np.uint8 and got.shape == tuple(scan["shape"]) == tuple((20, 24, 28)[a] for a in src)
        assert np.array_equal(got, ref_reorient(want, src, flip)), i          # voxel by voxel PointNet: the blend leaves it
        assert np.array_equal(h["affine"], scan["affine"]) and _affine_close(np.asarray(h["affine"], np.float64), affs[i])
        assert h["sform_code"] == scan["sform_code"] == 2 and h["qform_code"] == scan["qform_code"]
        assert list(h["pixdim"]) == list(scan["pixdim"])
        row = dict(zip(table[0], table[i + 1]))
        assert rows[i]["source_orient"] == row["source_orient"] == variant_code(src, flip) and row["orient"] == "RAS"
        assert row["source_shape"] == prep._fmt(got.shape) and row["grid_shape"] == "20 24 28"
        if i > 0:
            plan = prep.orient_plan(*prep.scan_orientation(affs[i]), "RAS", got.shape)[:2]
            assert ops.reoriented[2 * i - 2] == ((1,) + got.shape, "torch.float32") + plan
            assert ops.reoriented[2 * i - 1] == ((20, 24, 28), "torch.uint8") + prep.orient_inverse(*plan)
    if post:            # cleaned on the scan's own grid, after the map came back to it
        assert [c[0] for c in ops.cleaned] == [tuple((20, 24, 28)[a] for a in src) for src, _ in VARIANTS]
