"""The `prep` mission, host side (no GPU): nifti.read_image, what prep refuses, the geometry of resampling and
widening, the C-ABI rows of the effq_prep_* symbols, and the whole mission driven through a numpy stand-in for the
device ops (NumpyOps below, also the fp64 restatement the GPU tests compare the kernels with)."""
import gzip
import os
import pickle
import re
import struct

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, data as D, nifti, prep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = {np.uint8: 2, np.int16: 4, np.int32: 8, np.float32: 16, np.float64: 64, np.int8: 256, np.uint16: 512,
         np.uint32: 768}


# ---- NIfTI bytes built here, from nifti.FIELDS ----------------------------------------------------------------------
def nifti_bytes(a, end="<", slope=0.0, inter=0.0, affine=None, ndim=None, sform=2, pixdim=None):
    a = np.asarray(a)
    aff = np.eye(4) if affine is None else np.asarray(affine, dtype=np.float64)
    shape = list(a.shape)
    nd = len(shape) if ndim is None else ndim
    values = {"sizeof_hdr": (348,), "dim": [nd] + shape + [1] * (7 - len(shape)),
              "datatype": (CODES[a.dtype.type],), "bitpix": (8 * a.dtype.itemsize,),
              "pixdim": list(pixdim) if pixdim is not None else [1.0] * 8, "vox_offset": (352.0,),
              "scl_slope": (slope,), "scl_inter": (inter,), "xyzt_units": (2,), "qform_code": (0,),
              "sform_code": (sform,), "quatern": [0.0] * 6, "srow_x": list(aff[0]), "srow_y": list(aff[1]),
              "srow_z": list(aff[2]), "magic": (b"n+1\0",)}
    hdr = bytearray(348)
    for name, fmt, off in nifti.FIELDS:
        struct.pack_into(end + fmt, hdr, off, *values[name])
    return bytes(hdr) + b"\0" * 4 + a.astype(a.dtype.newbyteorder(end)).tobytes(order="F")


def write_scan(path, a, gz=True, **kw):
    raw = nifti_bytes(a, **kw)
    with open(path, "wb") as f:
        f.write(gzip.compress(raw, 1) if gz else raw)
    return str(path)


def ramp(dtype):
    r = np.arange(5 * 6 * 7, dtype=np.float64).reshape(5, 6, 7)
    if np.issubdtype(dtype, np.signedinteger) or np.issubdtype(dtype, np.floating):
        r = r - 100.0
    if dtype == np.int8:
        r = r * 0.5
    if np.issubdtype(dtype, np.floating):
        r = r * 0.37
    return r.astype(dtype)


@pytest.mark.parametrize("dtype", list(CODES))
@pytest.mark.parametrize("end", ["<", ">"])
@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("scale", [(0.0, 0.0), (0.5, -3.0)])
def test_read_image_round_trips(tmp_path, dtype, end, gz, scale):
    a = ramp(dtype)
    path = write_scan(tmp_path / ("a.nii.gz" if gz else "a.nii"), a, gz=gz, end=end, slope=scale[0], inter=scale[1])
    got, f = nifti.read_image(path)
    want = a.astype(np.float32)
    if scale[0] != 0.0:
        want = (a.astype(np.float64) * scale[0] + scale[1]).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == (5, 6, 7) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, want)
    assert f["shape"] == (5, 6, 7) and f["datatype"] == CODES[dtype]


def test_read_image_squeezes_one_volume_and_refuses_the_rest_and_read_nifti_still_refuses_int16(tmp_path):
    a = ramp(np.int16)
    p4 = write_scan(tmp_path / "four.nii", a[..., None], gz=False)
    assert np.array_equal(nifti.read_image(p4)[0], a.astype(np.float32))
    with pytest.raises(ValueError, match="four2"):
        nifti.read_image(write_scan(tmp_path / "four2.nii", np.stack([a, a], -1), gz=False))
    with pytest.raises(ValueError, match="two"):
        nifti.read_image(write_scan(tmp_path / "two.nii", a[0], gz=False))
    raw = bytearray(nifti_bytes(a))
    struct.pack_into("<h", raw, 70, 128)                                  # RGB24
    (tmp_path / "rgb.nii").write_bytes(bytes(raw))
    with pytest.raises(ValueError, match="datatype 128"):
        nifti.read_image(str(tmp_path / "rgb.nii"))
    with pytest.raises(ValueError, match="datatype 4"):
        nifti.read_nifti(write_scan(tmp_path / "i16.nii", a, gz=False))


def test_read_image_takes_the_affine_as_read_geometry_does(tmp_path):
    aff = np.array([[0.0, -0.8, 0.0, 10.0], [0.8, 0.0, 0.0, -20.0], [0.0, 0.0, 2.5, 30.0], [0, 0, 0, 1.0]])
    p = write_scan(tmp_path / "a.nii.gz", ramp(np.int16), affine=aff)
    f, g = nifti.read_image(p)[1], nifti.read_geometry(p)
    assert np.array_equal(f["affine"], g["affine"]) and f["spacing"] == g["spacing"]
    assert f["spacing"] == pytest.approx((0.8, 0.8, 2.5), rel=1e-6)
    p = write_scan(tmp_path / "b.nii.gz", ramp(np.int16), sform=0, pixdim=[1, 2.0, 3.0, 4.0, 0, 0, 0, 0])
    assert nifti.read_image(p)[1]["spacing"] == (2.0, 3.0, 4.0)


# ---- the numpy stand-in for the device ops: the fp64 restatement of csrc/prep.hip ------------------------------------
def ref_mask(x, mask):
    return np.ones(x.shape, bool) if mask == "all" else x != 0


def ref_bbox_moments(x, mask):
    m = ref_mask(x, mask)
    union = m.any(0)
    if mask == "all":
        box = [0, 0, 0] + [n - 1 for n in x.shape[1:]]
    elif not union.any():
        box = list(x.shape[1:]) + [-1, -1, -1]
    else:
        idx = np.nonzero(union)
        box = [int(i.min()) for i in idx] + [int(i.max()) for i in idx]
    count = [int(m[c].sum()) for c in range(x.shape[0])]
    total = [float(x[c][m[c]].astype(np.float64).sum()) for c in range(x.shape[0])]
    return box, count, total


def ref_sqdev(x, mean, mask):
    m = ref_mask(x, mask)
    return [float(((x[c][m[c]].astype(np.float64) - mean[c]) ** 2).sum()) for c in range(x.shape[0])]


def ref_standardise_crop(x, pmin, pmax, mean, std, mask):
    c = x[:, pmin[0]:pmax[0], pmin[1]:pmax[1], pmin[2]:pmax[2]]
    mu, sd = (np.asarray(v, dtype=np.float64).reshape(-1, 1, 1, 1) for v in (mean, std))
    y = ((c.astype(np.float64) - mu) / sd).astype(np.float32)
    return np.where(ref_mask(c, mask), y, np.float32(0.0))


def ref_axis_linear(n_out, f, n_in):
    """i0, i1 and the fp64 weight of i1 of every output index: s = (o + 0.5) f - 0.5 clamped to [0, n_in - 1]."""
    s = np.clip((np.arange(n_out, dtype=np.float64) + 0.5) * f - 0.5, 0.0, n_in - 1.0)
    i0 = np.floor(s).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_in - 1), s - i0


def ref_axis_nearest(n_out, f, n_in):
    return np.minimum(n_in - 1, np.floor((np.arange(n_out, dtype=np.float64) + 0.5) * f)).astype(np.int64)


def ref_resample_linear(x, factors, out_shape):
    """The trilinear formula in fp64 (weights and sums exact to fp64)."""
    (d0, d1, ld), (h0, h1, lh), (w0, w1, lw) = (ref_axis_linear(o, f, n) for o, f, n in zip(out_shape, factors, x.shape[1:]))
    v = x.astype(np.float64)
    ld, lh, lw = ld[:, None, None], lh[None, :, None], lw[None, None, :]
    g = lambda d, h, w: v[:, d[:, None, None], h[None, :, None], w[None, None, :]]
    a = (1 - lh) * ((1 - lw) * g(d0, h0, w0) + lw * g(d0, h0, w1)) + lh * ((1 - lw) * g(d0, h1, w0) + lw * g(d0, h1, w1))
    b = (1 - lh) * ((1 - lw) * g(d1, h0, w0) + lw * g(d1, h0, w1)) + lh * ((1 - lw) * g(d1, h1, w0) + lw * g(d1, h1, w1))
    return (1 - ld) * a + ld * b


def ref_resample_nearest(x, factors, out_shape):
    d, h, w = (ref_axis_nearest(o, f, n) for o, f, n in zip(out_shape, factors, x.shape[1:]))
    return x[:, d[:, None, None], h[None, :, None], w[None, None, :]]


class NumpyOps:
    """The prep_* methods of ops_prep.PrepOps (hip_ops.HipOps) on host tensors, for the orchestration tests only."""
    device = torch.device("cpu")

    def prep_window(self, x, lo, hi):
        x.copy_(torch.from_numpy(np.clip(x.numpy(), np.float32(lo), np.float32(hi))))
        return x

    def prep_resample(self, x, factors, out_shape, nearest=False):
        if nearest:
            return torch.from_numpy(np.ascontiguousarray(ref_resample_nearest(x.numpy(), factors, out_shape)))
        return torch.from_numpy(ref_resample_linear(x.numpy(), factors, out_shape).astype(np.float32))

    def prep_bbox_moments(self, x, mask="nonzero"):
        box, count, total = ref_bbox_moments(x.numpy(), mask)
        return torch.tensor(box, dtype=torch.int32), torch.tensor(count), torch.tensor(total, dtype=torch.float64)

    def prep_sqdev(self, x, mean, mask="nonzero"):
        return torch.tensor(ref_sqdev(x.numpy(), mean, mask), dtype=torch.float64)

    def prep_standardise_crop(self, x, pmin, pmax, mean, std, mask="nonzero"):
        return torch.from_numpy(np.ascontiguousarray(ref_standardise_crop(x.numpy(), pmin, pmax, mean, std, mask)))

    def prep_crop_u8(self, x, pmin, pmax):
        return torch.from_numpy(np.ascontiguousarray(
            x.numpy()[:, pmin[0]:pmax[0], pmin[1]:pmax[1], pmin[2]:pmax[2]]))

    def prep_union_mask(self, x, mask="nonzero"):
        return torch.from_numpy(ref_mask(x.numpy(), mask).any(0).astype(np.uint8))


# ---- synthetic subjects -----------------------------------------------------------------------------------------------
def brats_like(seed, shape=(20, 24, 28), margin=((2, 3), (4, 1), (3, 5))):
    """Four int16 modalities with a zero margin of differing width per side, and a label inside the body."""
    g = np.random.default_rng(seed)
    vols = np.zeros((4,) + shape, dtype=np.int16)
    body = tuple(slice(a, n - b) for (a, b), n in zip(margin, shape))
    for c in range(4):
        vols[c][body] = g.integers(200, 1200, size=vols[c][body].shape) * (1 + c)
    seg = np.zeros(shape, dtype=np.uint8)
    seg[body] = g.integers(0, 4, size=seg[body].shape)
    return vols, seg, body


def write_subjects(root, names, seeds, affine=None, **kw):
    """<root>/src/<name>_<mod>.nii.gz and the rows of a --src_list; returns {name: (vols, seg, body)}."""
    os.makedirs(os.path.join(root, "src"), exist_ok=True)
    rows, truth = [], {}
    for sn, seed in zip(names, seeds):
        vols, seg, body = brats_like(seed, **kw)
        cells = [sn]
        for c, m in enumerate(D.MODALITIES["brats"]):
            cells.append(os.path.join("src", f"{sn}_{m}.nii.gz"))
            write_scan(os.path.join(root, cells[-1]), vols[c], affine=affine)
        cells.append(os.path.join("src", f"{sn}_seg.nii.gz"))
        write_scan(os.path.join(root, cells[-1]), seg, affine=affine)
        rows.append(cells)
        truth[sn] = (vols, seg, body)
    return rows, truth


def write_list(path, rows, head=("subject", "flair", "t1", "t1ce", "t2", "seg")):
    with open(path, "w") as f:
        f.write(",".join(head) + "\n" + "".join(",".join(r) + "\n" for r in rows))
    return str(path)


def prep_args(**over):
    a = Cf.build_parser().parse_args(["prep", "--task", "brats"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


def written(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


# ---- the switches -----------------------------------------------------------------------------------------------------
def test_parser_knows_the_mission_and_its_switches_and_yaml_sets_them(tmp_path):
    a = Cf.build_parser().parse_args(["prep", "--task", "lits", "--src_list", "c.csv", "--data_dir", "o", "--val_every", "5",
                                      "--prep_mask", "all", "--prep_window", "-200,250", "--prep_spacing", "1,1,2",
                                      "--prep_min_size", "8,8,8", "--prep_no_crop"])
    assert a.prep_window == "-200,250" and prep.parse_window(a.prep_window, "lits") == (-200.0, 250.0)
    assert a.mission == "prep" and a.val_every == 5 and a.prep_no_crop is True and a.prep_spacing == "1,1,2"
    b = Cf.build_parser().parse_args(["ptq"])
    assert b.src_list is None and b.prep_mask is None and b.prep_no_crop is False
    cfg = tmp_path / "p.yaml"
    cfg.write_text("prep_spacing: '2,2,2'\nprep_mask: nonzero\n")
    a = Cf.merge_config(str(cfg), a)
    assert a.prep_spacing == "2,2,2" and a.prep_mask == "nonzero"          # YAML beats the command line
    assert prep.parse_window(None, "lits") == (-200.0, 250.0) and prep.parse_window(None, "brats") is None
    assert prep.parse_window("none", "lits") is None and prep.parse_window("-5,7.5", "brats") == (-5.0, 7.5)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_src_list_refusals_name_the_row_and_write_nothing(tmp_path):
    root = str(tmp_path)
    rows, _ = write_subjects(root, ["a", "b"], [1, 2])
    out = os.path.join(root, "out")

    def refused(rows, named, head=("subject", "flair", "t1", "t1ce", "t2", "seg")):
        lst = write_list(tmp_path / "cases.csv", rows, head)
        with pytest.raises(SystemExit) as e:
            prep.run(prep_args(src_list=lst, data_dir=out, prep_min_size="8,8,8"), ops=NumpyOps())
        assert all(n in str(e.value) for n in named), str(e.value)
        assert not os.path.exists(out)

    refused(rows, ("row 1", "adc"), head=("subject", "flair", "t1", "adc", "t2", "seg"))
    refused(rows, ("row 1",), head=("subject", "flair", "t1", "t1", "t2", "seg"))
    refused(rows + [rows[0]], ("row 4", "subject a"))
    gone = [list(rows[0]), list(rows[1])]
    gone[1][2] = os.path.join("src", "nowhere.nii.gz")
    refused(gone, ("row 3", "subject b", "nowhere.nii.gz"))
    bad = [list(rows[0])]
    bad[0][0] = "x/y"
    refused(bad, ("row 2", "x/y"))


def test_mismatched_shapes_and_affines_within_a_subject_are_refused_before_anything_is_written(tmp_path):
    root, out = str(tmp_path), str(tmp_path / "out")
    rows, truth = write_subjects(root, ["a", "b"], [1, 2])
    lst = write_list(tmp_path / "cases.csv", rows)
    write_scan(os.path.join(root, rows[1][3]), truth["b"][0][2][:, :, :-1])           # b's t1ce: one slice short
    with pytest.raises(SystemExit) as e:
        prep.run(prep_args(src_list=lst, data_dir=out, prep_min_size="8,8,8"), ops=NumpyOps())
    assert "subject b" in str(e.value) and "t1ce" in str(e.value) and not os.path.exists(out)
    shifted = np.eye(4)
    shifted[0, 3] = 0.01                                                               # 10 um: more than 1e-3 mm
    write_scan(os.path.join(root, rows[1][3]), truth["b"][0][2], affine=shifted)
    with pytest.raises(SystemExit) as e:
        prep.run(prep_args(src_list=lst, data_dir=out, prep_min_size="8,8,8"), ops=NumpyOps())
    assert "subject b" in str(e.value) and "affine" in str(e.value) and not os.path.exists(out)
    turned = np.eye(4)
    turned[1, 1] = 1.001                                                               # 1e-3 relative: more than 1e-4
    write_scan(os.path.join(root, rows[1][3]), truth["b"][0][2], affine=turned)
    with pytest.raises(SystemExit) as e:
        prep.run(prep_args(src_list=lst, data_dir=out, prep_min_size="8,8,8"), ops=NumpyOps())
    assert "subject b" in str(e.value) and not os.path.exists(out)
    near = np.eye(4)
    near[0, 3], near[1, 1] = 5e-4, 1.00005                                             # within both tolerances
    write_scan(os.path.join(root, rows[1][3]), truth["b"][0][2], affine=near)
    prep.run(prep_args(src_list=lst, data_dir=out, prep_min_size="8,8,8"), ops=NumpyOps())
    assert os.path.isfile(os.path.join(out, "t1ce", "b.npy"))


def test_a_grid_smaller_than_the_least_size_and_an_all_zero_subject_are_refused_by_name(tmp_path):
    root, out = str(tmp_path), str(tmp_path / "out")
    rows, truth = write_subjects(root, ["a", "b"], [1, 2])
    lst = write_list(tmp_path / "cases.csv", rows)
    with pytest.raises(SystemExit) as e:                                   # the default: the task's patch, 128^3
        prep.run(prep_args(src_list=lst, data_dir=out), ops=NumpyOps())
    assert "subject a" in str(e.value) and "--prep_min_size" in str(e.value) and not os.path.exists(out)
    with pytest.raises(SystemExit) as e:
        prep.run(prep_args(src_list=lst, data_dir=out, prep_min_size="8,8,29"), ops=NumpyOps())
    assert "subject a" in str(e.value) and not os.path.exists(out)
    for c in range(1, 5):
        write_scan(os.path.join(root, rows[0][c]), np.zeros((20, 24, 28), np.int16))
    with pytest.raises(SystemExit) as e:
        prep.run(prep_args(src_list=lst, data_dir=out, split_dir=str(tmp_path / "split"), val_every=2,
                           prep_min_size="8,8,8"), ops=NumpyOps())
    assert "subject a" in str(e.value) and "zero" in str(e.value)
    assert written(out) == [] and not os.path.exists(tmp_path / "split")
    # a constant modality: the modality is named
    flat = np.zeros((20, 24, 28), np.int16)
    flat[5:15, 5:15, 5:15] = 7
    for c in range(1, 5):
        write_scan(os.path.join(root, rows[0][c]), truth["a"][0][c - 1] if c != 2 else flat)
    with pytest.raises(SystemExit) as e:
        prep.run(prep_args(src_list=lst, data_dir=out, prep_min_size="8,8,8"), ops=NumpyOps())
    assert "subject a" in str(e.value) and "t1" in str(e.value) and written(out) == []


# ---- geometry ---------------------------------------------------------------------------------------------------------
def test_resample_extents_affine_and_widening_match_hand_computed_cases():
    assert prep.resample_extent(155, 2.0) == 78            # 77.5 rounds to the even 78
    assert prep.resample_extent(5, 2.0) == 2               # 2.5 rounds to the even 2
    assert prep.resample_extent(30, 1.6 / 2.5) == 47       # 46.875
    assert prep.resample_extent(48, 2.0) == 24 and prep.resample_extent(7, 0.5) == 14
    assert prep.resample_extent(3, 100.0) == 1             # never below one voxel
    aff = np.array([[0.8, 0, 0, -10.0], [0, 0.8, 0, 5.0], [0, 0, 2.5, 100.0], [0, 0, 0, 1.0]])
    got = prep.resample_affine(aff, (2.0, 2.0, 0.64))
    want = np.array([[1.6, 0, 0, -10.0 + 0.8 * 0.5], [0, 1.6, 0, 5.0 + 0.8 * 0.5], [0, 0, 1.6, 100.0 + 2.5 * -0.18],
                     [0, 0, 0, 1.0]])
    assert np.allclose(got, want, rtol=0, atol=1e-12)
    # output voxel 0 lies at source coordinate (0 + 0.5) f - 0.5
    assert np.allclose(got @ [0, 0, 0, 1], aff @ [0.5, 0.5, -0.18, 1], atol=1e-12)
    w = prep.widen_box
    assert w((10, 10, 10), (14, 15, 30), (40, 40, 40), (8, 8, 8)) == ((8, 8, 10), (16, 16, 30))   # +4 even, +3 odd: low side
    assert w((10,), (15,), (40,), (8,)) == ((8,), (16,))              # 3 more: two below, one above
    assert w((1,), (4,), (40,), (8,)) == ((0,), (8,))                 # clamped at the low border
    assert w((36,), (40,), (40,), (8,)) == ((32,), (40,))             # and at the high one
    assert w((0,), (40,), (40,), (40,)) == ((0,), (40,))
    with pytest.raises(ValueError):
        w((0,), (4,), (6,), (8,))


# ---- the symbols ------------------------------------------------------------------------------------------------------
def test_prep_symbols_in_header_and_lib_have_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = re.findall(r"\bint (effq_prep_\w+)\s*\((.*?)\)\s*;", code, flags=re.S)
    names = {n for n, _ in found}
    assert names == {n for n in _lib.SIGNATURES if n.startswith("effq_prep_")}
    assert {"effq_prep_window", "effq_prep_resample", "effq_prep_bbox_moments", "effq_prep_sqdev",
            "effq_prep_standardise_crop"} <= names

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return _lib._P
        if decl.startswith("long long"):
            return _lib._LL
        return {"int": _lib._I, "float": _lib._F, "double": _lib._D, "size_t": _lib._SZ}[decl.split()[0]]
    for name, args in found:
        res, got = _lib.SIGNATURES[name]
        assert res == _lib._I and got == [ctype(a) for a in args.split(",")], name
    ws = re.search(r"#define EFFQ_PREP_WS_BYTES (.*)", code).group(1)
    ws = ws.replace("EFFQ_PREP_MAX_MODALITIES", str(_lib.PREP_MAX_MODALITIES))
    assert re.fullmatch(r"[\d\s()*+]+", ws) and eval(ws) == _lib.PREP_WS_BYTES
    assert "prep.hip" in open(os.path.join(ROOT, "efficientq_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "efficientq_amd", "csrc", "prep.hip")).read()
    assert not re.search(r"atomic\w*\s*\(", re.sub(r"//.*", "", src))       # deterministic: no atomics at all


# ---- the whole mission on the host --------------------------------------------------------------------------------------
def test_whole_mission_writes_what_the_ptq_mission_reads_and_a_second_run_merges(tmp_path):
    root = str(tmp_path)
    out, split = os.path.join(root, "out"), os.path.join(root, "split")
    aff = np.array([[1.5, 0, 0, -3.0], [0, 1.0, 0, 4.0], [0, 0, 2.0, 5.0], [0, 0, 0, 1.0]])
    rows, truth = write_subjects(root, ["s3", "s1", "s2"], [3, 1, 2], affine=aff)
    rows[1][5] = ""                                                           # s1 has no label
    lst = write_list(tmp_path / "cases.csv", rows)
    got = prep.run(prep_args(src_list=lst, data_dir=out, split_dir=split, val_every=2, prep_min_size="8,8,8"),
                   ops=NumpyOps())
    assert [r["subject"] for r in got] == ["s1", "s2", "s3"]
    assert open(os.path.join(split, "round1", "train.txt")).read().split() == ["s1", "s3"]
    assert open(os.path.join(split, "round1", "val.txt")).read().split() == ["s2"]
    assert not os.path.exists(os.path.join(out, "seg", "s1.npy")) and os.path.isfile(os.path.join(out, "seg", "s2.npy"))
    assert not [f for f in written(out) if f.endswith(".tmp")]
    info = pickle.load(open(os.path.join(out, D.RESTORE_FILE), "rb"))
    assert sorted(info) == ["s1", "s2", "s3"]
    assert all(type(v) is int for kw in info.values() for k in ("pmin", "pmax", "shape") for v in kw[k])
    assert all(type(kw[k]) is tuple for kw in info.values() for k in ("pmin", "pmax", "shape"))
    lines = open(os.path.join(out, D.SN_FN_FILE)).read().splitlines()
    assert [ln.split(",")[0] for ln in lines] == ["s1", "s2", "s3"]
    assert lines[0].split(",")[1] == os.path.join(root, "src", "s1_flair.nii.gz")
    # every subject: the restored crop is the standardised full volume, background exactly zero
    for sn in ("s1", "s2", "s3"):
        vols, seg, body = truth[sn]
        assert info[sn]["pmin"] == tuple(s.start for s in body) and info[sn]["pmax"] == tuple(s.stop for s in body)
        assert info[sn]["shape"] == (20, 24, 28)
        for c, m in enumerate(D.MODALITIES["brats"]):
            v = vols[c].astype(np.float64)
            inside = v[v != 0]
            full = np.where(v != 0, ((v - inside.mean()) / inside.std()).astype(np.float32), np.float32(0))
            arr = np.load(os.path.join(out, m, f"{sn}.npy"))
            assert arr.dtype == np.float32
            back = D.restore_crop(arr, **info[sn])
            assert np.allclose(back, full, rtol=0, atol=2e-6) and np.array_equal(back == 0, v == 0)
        if sn != "s1":
            lab = np.load(os.path.join(out, "seg", f"{sn}.npy"))
            assert lab.dtype == np.uint8 and np.array_equal(D.restore_crop(lab, **info[sn]), seg)
    # the ptq mission's own readers accept it (s1 carries no label: the labelled cube is built from the val subject)
    args = Cf.make_args(dict(Cf.TINY_NET, task="brats", nMod=4, nClass=4, multi_label="brats"), 4, 4, data_dir=out,
                        split_dir=split, access_type="npy", merge_type=None, patch_size="8", src_geom=True)
    cube = D.get_data_cube(args)
    assert cube.val_sn == ["s2"] and cube.geometry[0]["pmin"] == info["s2"]["pmin"]
    assert np.allclose(cube.geometry[0]["affine"], aff) and cube.geometry[0]["spacing"] == pytest.approx((1.5, 1.0, 2.0))
    image, label = next(iter(cube.valloader))
    assert image.shape[1] == 4 and label.shape[1] == 3
    geo = D.read_source_geometry(out, ["s1", "s2", "s3"], "npy", "flair")
    assert [g["source_shape"] for g in geo] == [(20, 24, 28)] * 3
    table = [ln.split(",") for ln in open(os.path.join(out, prep.PREP_CSV)).read().splitlines()]
    assert table[0][:7] == ["subject", "source_shape", "source_spacing", "grid_shape", "grid_spacing", "pmin", "pmax"]
    assert table[0][7:10] == ["flair_count", "flair_mean", "flair_std"] and len(table[0]) == 7 + 12
    assert [r[0] for r in table[1:]] == ["s1", "s2", "s3"] and table[1][1] == "20 24 28"
    assert table[1][2] == "1.5 1 2" and table[1][5] == " ".join(str(s.start) for s in truth["s1"][2])

    # a second run of one more subject (and s2 again, uncropped) merges into the index files
    rows2, truth2 = write_subjects(os.path.join(root, "more"), ["s0"], [7])
    lst2 = write_list(os.path.join(root, "more", "cases.csv"), rows2)
    with pytest.raises(SystemExit) as e:                                      # the split exists already
        prep.run(prep_args(src_list=lst2, data_dir=out, split_dir=split, val_every=2, prep_min_size="8,8,8"),
                 ops=NumpyOps())
    assert "train.txt" in str(e.value) and not os.path.exists(os.path.join(out, "flair", "s0.npy"))
    prep.run(prep_args(src_list=lst2, data_dir=out, prep_min_size="8,8,8"), ops=NumpyOps())
    info2 = pickle.load(open(os.path.join(out, D.RESTORE_FILE), "rb"))
    assert sorted(info2) == ["s0", "s1", "s2", "s3"] and all(info2[k] == info[k] for k in info)
    lines2 = open(os.path.join(out, D.SN_FN_FILE)).read().splitlines()
    assert [ln.split(",")[0] for ln in lines2] == ["s0", "s1", "s2", "s3"] and lines2[1:] == lines
    assert len(D.read_source_geometry(out, ["s0", "s1", "s2", "s3"], "npy", "flair")) == 4
    table2 = open(os.path.join(out, prep.PREP_CSV)).read().splitlines()
    assert [r.split(",")[0] for r in table2[1:]] == ["s0", "s1", "s2", "s3"]
    keep = write_list(tmp_path / "again.csv", [r for r in rows if r[0] == "s2"])
    prep.run(prep_args(src_list=keep, data_dir=out, prep_min_size="8,8,8", prep_no_crop=True, access_type="npz"),
             ops=NumpyOps())
    info3 = pickle.load(open(os.path.join(out, D.RESTORE_FILE), "rb"))
    assert sorted(info3) == ["s0", "s1", "s3"]                               # the newer, uncropped s2 has no entry
    with np.load(os.path.join(out, "t2", "s2.npz")) as z:
        assert z["arr_0"].shape == (20, 24, 28)


def test_whole_mission_on_a_resampled_grid_names_the_grid_image(tmp_path):
    root, out = str(tmp_path), str(tmp_path / "out")
    aff = np.diag([1.0, 1.0, 2.0, 1.0])
    rows, truth = write_subjects(root, ["a"], [5], affine=aff)
    lst = write_list(tmp_path / "cases.csv", rows)
    prep.run(prep_args(src_list=lst, data_dir=out, prep_spacing="2,2,2", prep_min_size="4,4,4"), ops=NumpyOps())
    assert open(os.path.join(out, D.SN_FN_FILE)).read() == "a,grid/a.nii.gz\n"
    g = nifti.read_geometry(os.path.join(out, "grid", "a.nii.gz"))
    assert g["shape"] == (10, 12, 28) and g["spacing"] == pytest.approx((2.0, 2.0, 2.0))
    assert np.allclose(g["affine"], prep.resample_affine(aff, (2.0, 2.0, 1.0)))
    union, _ = nifti.read_nifti(os.path.join(out, "grid", "a.nii.gz"))
    geo = D.read_source_geometry(out, ["a"], "npy", "seg")[0]
    arr = np.load(os.path.join(out, "flair", "a.npy"))
    assert arr.shape == tuple(b - a for a, b in zip(geo["pmin"], geo["pmax"]))
    back = D.restore_crop(arr, geo["pmin"], geo["pmax"], geo["source_shape"])
    assert np.array_equal(back != 0, union != 0) or (back != 0).sum() <= (union != 0).sum()
    assert set(np.unique(np.load(os.path.join(out, "seg", "a.npy")))) <= {0, 1, 2, 3}
