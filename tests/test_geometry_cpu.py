"""Source geometry of the validation, host side (no GPU): the fp32 yardstick of the weighted distance transform (brute
force over all sites against the separable form, bit for bit, and against scipy where it imports), nifti.read_geometry
on files of every kind it promises to read, write_nifti(..., geometry=), sn_fn.txt and the restore pickle, every error
of --src_geom, evaluate.surface_metrics_mm and the _mm columns of metrics.csv, and the C-ABI rows of the new kernels."""
import csv
import gzip
import math
import os
import pickle
import re
import struct

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, data as D, evaluate as E, nifti as N
from tests.test_seg_eval_cpu import write_dataset
from tests.test_seg_surface_cpu import ref_edt_sq, ref_surface

try:
    from scipy import ndimage
except ImportError:          # the extra assertions against scipy are then not made
    ndimage = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SPACINGS = [(1.0, 1.0, 1.0), (5.0, 0.7421875, 0.7421875), (2.5, 0.683, 0.683), (0.8, 0.9766, 1.37)]
SCIPY_RTOL = 2.0 ** -21      # five fp32 roundings: (1 + 2^-24)^5 - 1 < 2^-21


# ---- the yardstick ------------------------------------------------------------------------------------------------
def weights(spacing):
    """What the host hands the kernels: float32(float64(spacing_a) ** 2) per axis (d, h, w)."""
    return tuple(F32(np.float64(s) ** 2) for s in spacing)


def ref_edt_mm_brute(sites, spacing):
    """min over the sites s of fl(fl(fl(ww dw^2) + fl(wh dh^2)) + fl(wd dd^2)), every operation in numpy fp32 (no fused
    multiply-add: each ufunc rounds once); +inf without a site."""
    s = np.asarray(sites) != 0
    assert s.ndim == 3
    wd, wh, ww = weights(spacing)
    best = np.full(s.size, np.inf, F32)
    pts = np.argwhere(s)
    vox = np.indices(s.shape).reshape(3, -1).T
    for k in range(0, len(pts), 128):
        diff = vox[:, None, :] - pts[None, k:k + 128, :]
        sq = (diff * diff).astype(F32)                       # < 2^24: exact
        e = (ww * sq[..., 2] + wh * sq[..., 1]) + wd * sq[..., 0]
        assert e.dtype == F32
        best = np.minimum(best, e.min(1))
    return best.reshape(s.shape)


def ref_edt_mm_lines(sites, spacing):
    """The same map axis by axis (w, then h, then d), min_j fl(g(j) + fl(wa (i - j)^2)) over whole lines in numpy fp32:
    for volumes too large for the brute force."""
    s = np.asarray(sites) != 0
    wd, wh, ww = weights(spacing)
    g = np.where(s, F32(0), F32(np.inf)).astype(F32)
    for ax, wa in ((2, ww), (1, wh), (0, wd)):
        n = s.shape[ax]
        g = np.moveaxis(g, ax, 0)
        i = np.arange(n)
        out = np.full_like(g, np.inf)
        for j in range(n):
            c = (wa * ((i - j) ** 2).astype(F32)).reshape((n,) + (1,) * (g.ndim - 1))
            out = np.minimum(out, g[j][None] + c)
        assert out.dtype == F32
        g = np.moveaxis(out, 0, ax)
    return np.ascontiguousarray(g)


def ref_surface_counts_mm(pred, gt, spacing, edt=ref_edt_mm_lines):
    """What effq_seg_surface_mm returns for one class: ([nP, nL], [max_PL, max_LP, qlo, qhi] fp32, [sum_PL, sum_LP])."""
    sp, sl = ref_surface(pred), ref_surface(gt)
    n_p, n_l = int(sp.sum()), int(sl.sum())
    e_pl = np.sort(edt(sl, spacing)[sp]) if n_l else np.zeros(0, F32)
    e_lp = np.sort(edt(sp, spacing)[sl]) if n_p else np.zeros(0, F32)
    sq = [F32(e_pl.max()) if len(e_pl) else F32(0), F32(e_lp.max()) if len(e_lp) else F32(0), F32(0), F32(0)]
    if n_p and n_l:
        pooled = np.sort(np.hstack([e_pl, e_lp]))
        n = len(pooled)
        lo = 95 * (n - 1) // 100
        sq[2:] = [pooled[lo], pooled[min(lo + 1, n - 1)]]
    return [n_p, n_l], sq, [float(np.sqrt(e_pl.astype(np.float64)).sum()), float(np.sqrt(e_lp.astype(np.float64)).sum())]


def ref_surface_metrics_mm(pred, gt, spacing, edt=ref_edt_mm_lines):
    """(hd, hd95, assd) in mm of one class from the definitions, numpy.percentile included."""
    sp, sl = ref_surface(pred), ref_surface(gt)
    if not sp.any() and not sl.any():
        return (0.0, 0.0, 0.0)
    if not sp.any() or not sl.any():
        return (math.sqrt(sum((e * s) ** 2 for e, s in zip(sp.shape, spacing))),) * 3
    d_pl = np.sqrt(edt(sl, spacing)[sp].astype(np.float64))
    d_lp = np.sqrt(edt(sp, spacing)[sl].astype(np.float64))
    pooled = np.hstack([d_pl, d_lp])
    return (float(pooled.max()), float(np.percentile(pooled, 95)), float((d_pl.mean() + d_lp.mean()) / 2))


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("density", [0.02, 0.3])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_brute_force_and_line_maps_agree_bit_for_bit(spacing, density):
    s = np.random.default_rng(5).random((9, 14, 19)) < density
    brute, lines = ref_edt_mm_brute(s, spacing), ref_edt_mm_lines(s, spacing)
    assert brute.dtype == lines.dtype == F32
    assert np.array_equal(bits(brute), bits(lines))
    assert (brute[s] == 0).all() and np.isfinite(brute).all()
    if ndimage is not None:
        want = ndimage.distance_transform_edt(~s, sampling=spacing) ** 2
        ok = want > 0
        rel = np.abs(brute.astype(np.float64)[ok] - want[ok]) / want[ok]
        print("worst relative difference to scipy", rel.max())
        assert rel.max() <= SCIPY_RTOL and (brute[~ok] == 0).all()


def test_a_volume_without_sites_is_infinite_everywhere():
    z = np.zeros((3, 4, 5))
    assert np.isposinf(ref_edt_mm_brute(z, SPACINGS[1])).all() and np.isposinf(ref_edt_mm_lines(z, SPACINGS[1])).all()


@pytest.mark.parametrize("density", [0.02, 0.3])
def test_unit_spacing_gives_the_integer_map_as_floats(density):
    s = np.random.default_rng(3).random((11, 13, 17)) < density
    want = ref_edt_sq(s)
    for got in (ref_edt_mm_brute(s, (1, 1, 1)), ref_edt_mm_lines(s, (1, 1, 1))):
        assert np.array_equal(got, want.astype(F32)) and np.array_equal(got.astype(np.int64), want)


def test_anisotropic_boxes_have_closed_form_distances():
    shape, sp = (12, 14, 16), (5.0, 0.7421875, 0.7421875)
    a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    a[2:8, 2:9, 2:9] = 1
    b[3:9, 2:9, 2:9] = 1                                # shifted by one slice: 5 mm, or a few steps in the plane
    hd, hd95, assd = ref_surface_metrics_mm(a, b, sp)
    assert hd == 5.0 and 0 < assd < hd95 <= hd
    cnt, sq, sums = ref_surface_counts_mm(a, b, sp)
    got = E.surface_metrics_mm(torch.tensor([cnt]), torch.tensor([[float(v) for v in sq]]),
                               torch.tensor([sums], dtype=torch.float64), shape, sp)[0].tolist()
    assert all(abs(g - w) <= 1e-12 * w for g, w in zip(got, (hd, hd95, assd)))


# ---- nifti.read_geometry --------------------------------------------------------------------------------------------
def pack_header(end, shape, datatype, bitpix, pixdim, qform_code, sform_code, quatern, srows, xyzt_units=10):
    """A NIfTI-1 header packed by hand, field by field at the offsets of nifti1.h."""
    h = bytearray(352)
    struct.pack_into(end + "i", h, 0, 348)
    struct.pack_into(end + "8h", h, 40, len(shape), *shape, *([1] * (7 - len(shape))))
    struct.pack_into(end + "hh", h, 70, datatype, bitpix)
    struct.pack_into(end + "8f", h, 76, *pixdim)
    struct.pack_into(end + "f", h, 108, 352.0)
    h[123] = xyzt_units                                  # 10 = millimetres and seconds
    struct.pack_into(end + "hh", h, 252, qform_code, sform_code)
    struct.pack_into(end + "6f", h, 256, *quatern)
    for k in range(3):
        struct.pack_into(end + "4f", h, 280 + 16 * k, *srows[k])
    h[344:348] = b"n+1\0"
    return bytes(h)


def f32(v):
    return float(F32(v))


def qform_expected(quatern, pixdim):
    """nifti1.h METHOD 2 on the float32 fields, written out entry by entry."""
    b, c, d = (f32(v) for v in quatern[:3])
    a = math.sqrt(max(0.0, 1.0 - (b * b + c * c + d * d)))
    qfac = -1.0 if f32(pixdim[0]) < 0 else 1.0
    pi, pj, pk = f32(pixdim[1]), f32(pixdim[2]), f32(pixdim[3]) * qfac
    m = np.eye(4)
    m[0, :3] = [(a * a + b * b - c * c - d * d) * pi, 2 * (b * c - a * d) * pj, 2 * (b * d + a * c) * pk]
    m[1, :3] = [2 * (b * c + a * d) * pi, (a * a + c * c - b * b - d * d) * pj, 2 * (c * d - a * b) * pk]
    m[2, :3] = [2 * (b * d - a * c) * pi, 2 * (c * d + a * b) * pj, (a * a + d * d - b * b - c * c) * pk]
    m[:3, 3] = [f32(v) for v in quatern[3:]]
    return m


ZERO_ROWS = [(0.0,) * 4] * 3
QCASES = {
    # 90 degrees about k: b = c = 0, d = sqrt(1/2)
    "rot90": dict(quatern=(0.0, 0.0, math.sqrt(0.5), -90.0, 126.0, -72.0), pixdim=(1.0, 0.7, 0.8, 5.0, 0, 0, 0, 0)),
    "oblique_qfac": dict(quatern=(0.1, -0.2, 0.3, 12.5, -3.25, 40.0), pixdim=(-1.0, 0.9766, 0.9766, 2.5, 0, 0, 0, 0)),
}


@pytest.mark.parametrize("case", sorted(QCASES))
@pytest.mark.parametrize("end,gz,datatype,bitpix", [("<", False, 16, 32), (">", True, 4, 16), ("<", True, 4, 16),
                                                     (">", False, 16, 32)])
def test_read_geometry_of_a_qform_only_header(tmp_path, case, end, gz, datatype, bitpix):
    q = QCASES[case]
    shape = (7, 9, 4)
    raw = pack_header(end, shape, datatype, bitpix, q["pixdim"], 1, 0, q["quatern"], ZERO_ROWS)
    raw += b"\0" * (7 * 9 * 4 * bitpix // 8)
    path = str(tmp_path / ("g.nii.gz" if gz else "g.nii"))
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(raw)
    g = N.read_geometry(path)
    want = qform_expected(q["quatern"], q["pixdim"])
    assert g["shape"] == shape and g["qform_code"] == 1 and g["sform_code"] == 0 and g["datatype"] == datatype
    assert np.allclose(g["affine"], want, rtol=0, atol=1e-12)
    # a rotation keeps lengths: the spacing is |pixdim| whatever the quaternion
    assert np.allclose(g["spacing"], [f32(v) for v in q["pixdim"][1:4]], rtol=1e-12, atol=0)
    if case == "rot90":                                   # i runs along +y, j along -x
        assert np.allclose(g["affine"][:3, :3], [[0, -f32(0.8), 0], [f32(0.7), 0, 0], [0, 0, 5.0]], atol=1e-7)
    else:
        assert np.linalg.det(g["affine"][:3, :3]) < 0     # qfac -1: a left-handed grid
    with pytest.raises(ValueError):
        N.read_nifti(path)                                # the voxel reader keeps its uint8 / uint16 restriction


def test_read_geometry_prefers_sform_then_qform_then_pixdim(tmp_path):
    rows = [(0.0, 0.0, 5.0, 1.0), (0.7421875, 0.0, 0.0, 2.0), (0.0, -0.7421875, 0.0, 3.0)]
    pixdim = (1.0, 2.0, 3.0, 4.0, 0, 0, 0, 0)
    quat = (0.0, 0.0, 0.0, 9.0, 8.0, 7.0)
    for codes, want_spacing in (((1, 2), (0.7421875, 0.7421875, 5.0)), ((1, 0), (2.0, 3.0, 4.0)),
                                ((0, 0), (2.0, 3.0, 4.0))):
        path = str(tmp_path / f"s{codes[0]}{codes[1]}.nii")
        with open(path, "wb") as f:
            f.write(pack_header("<", (3, 4, 5), 2, 8, pixdim, codes[0], codes[1], quat, rows) + b"\0" * 60)
        g = N.read_geometry(path)
        assert g["spacing"] == want_spacing, codes
        if codes[1]:
            assert np.array_equal(g["affine"], np.array(rows + [(0, 0, 0, 1)], dtype=np.float64))
        elif codes[0]:
            assert np.array_equal(g["affine"], np.array([[2.0, 0, 0, 9], [0, 3, 0, 8], [0, 0, 4, 7], [0, 0, 0, 1]]))
        else:
            assert np.array_equal(g["affine"], np.diag([2.0, 3.0, 4.0, 1.0]))


def test_read_geometry_rejects_other_files(tmp_path):
    p = tmp_path / "x.nii"
    p.write_bytes(b"\0" * 400)
    with pytest.raises(ValueError):
        N.read_geometry(str(p))
    p.write_bytes(b"\0" * 10)
    with pytest.raises(ValueError):
        N.read_geometry(str(p))
    two_file = bytearray(pack_header("<", (3, 4, 5), 2, 8, (1,) * 8, 0, 0, (0,) * 6, ZERO_ROWS))
    two_file[344:348] = b"ni1\0"
    p.write_bytes(bytes(two_file))
    with pytest.raises(ValueError):
        N.read_geometry(str(p))


def test_only_the_header_of_a_gzip_file_is_inflated(tmp_path):
    """A file cut off after its first 2 KiB still gives its geometry: the data block is never reached."""
    rng = np.random.default_rng(0)
    a = rng.integers(0, 60000, size=(40, 50, 30)).astype(np.uint16)
    path = str(tmp_path / "big.nii.gz")
    N.write_nifti(path, a, np.diag([2.0, 3.0, 4.0, 1.0]))
    whole = open(path, "rb").read()
    assert len(whole) > 50000
    open(path, "wb").write(whole[:2048])
    g = N.read_geometry(path)
    assert g["shape"] == (40, 50, 30) and g["spacing"] == (2.0, 3.0, 4.0)


def test_write_nifti_with_a_geometry_round_trips(tmp_path):
    q = QCASES["oblique_qfac"]
    rows = [(0.7421875, 0.0, 0.0, -90.0), (0.0, 0.7421875, 0.0, 126.0), (0.0, 0.0, 5.0, -72.0)]
    src = str(tmp_path / "src.nii")
    with open(src, "wb") as f:
        f.write(pack_header(">", (6, 5, 4), 16, 32, q["pixdim"], 1, 2, q["quatern"], rows) + b"\0" * 480)
    g = N.read_geometry(src)
    a = np.arange(120, dtype=np.uint16).reshape(6, 5, 4)
    for name in ("m.nii.gz", "m.nii"):
        out = str(tmp_path / name)
        N.write_nifti(out, a, geometry=g)
        g2 = N.read_geometry(out)
        for k in ("shape", "pixdim", "xyzt_units", "qform_code", "sform_code", "quatern", "srow_x", "srow_y", "srow_z",
                  "spacing"):
            assert g2[k] == g[k], k
        assert g2["xyzt_units"] == 10
        assert np.array_equal(g2["affine"], g["affine"]) and g2["datatype"] == 512
        back, f = N.read_nifti(out)
        assert np.array_equal(back, a) and f["qform_code"] == 1 and f["sform_code"] == 2
    with pytest.raises(ValueError):
        N.write_nifti(out, a, np.eye(4), geometry=g)
    with pytest.raises(ValueError):
        N.write_nifti(out, a[:5], geometry=g)


def test_write_nifti_without_a_geometry_gives_the_bytes_it_always_gave(tmp_path):
    a = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
    aff = np.array([[0.0, 0, 5, 1], [0.75, 0, 0, 2], [0, -0.75, 0, 3], [0, 0, 0, 1]])
    for affine in (None, aff):
        use = np.eye(4) if affine is None else affine
        h = bytearray(348)
        struct.pack_into("<i", h, 0, 348)
        h[38:39] = b"r"
        struct.pack_into("<8h", h, 40, 3, 2, 3, 4, 1, 1, 1, 1)
        struct.pack_into("<hh", h, 70, 2, 8)
        struct.pack_into("<8f", h, 76, *([1.0] * 8))
        struct.pack_into("<f", h, 108, 352.0)
        struct.pack_into("<hh", h, 252, 0, 2)
        struct.pack_into("<6f", h, 256, 0.0, 0.0, 0.0, *use[:3, 3])
        for k in range(3):
            struct.pack_into("<4f", h, 280 + 16 * k, *use[k])
        h[344:348] = b"n+1\0"
        want = bytes(h) + b"\0" * 4 + a.tobytes(order="F")
        assert N.encode_nifti(a, affine) == want
        N.write_nifti(str(tmp_path / "p.nii"), a, affine)
        assert open(tmp_path / "p.nii", "rb").read() == want
        N.write_nifti(str(tmp_path / "p.nii.gz"), a, affine)
        assert gzip.decompress(open(tmp_path / "p.nii.gz", "rb").read()) == want


# ---- sn_fn.txt, the restore pickle, --src_geom ------------------------------------------------------------------------
SRC_ROWS = [(0.0, 0.0, 5.0, 1.0), (0.7421875, 0.0, 0.0, 2.0), (0.0, -0.7421875, 0.0, 3.0)]


def write_sources(data_dir, subjects, shape, crop=None, rows=SRC_ROWS, relative=True):
    """Source headers (float32 images of `shape`, spacing (0.7421875, 0.7421875, 5)), sn_fn.txt and, with `crop` =
    {subject: (pmin, pmax)}, the restore pickle, in the reference's layout."""
    os.makedirs(os.path.join(data_dir, "src"), exist_ok=True)
    lines = []
    for k, sn in enumerate(subjects):
        path = os.path.join(data_dir, "src", f"{sn}.nii.gz")
        with gzip.open(path, "wb") as f:
            f.write(pack_header("<>"[k % 2], shape, 16, 32, (1.0, 0.7421875, 0.7421875, 5.0, 0, 0, 0, 0), 1, 1,
                                (0.5, 0.5, 0.5, 1.0, 2.0, 3.0), rows))
        lines.append(f"{sn},{os.path.join('src', sn + '.nii.gz') if relative else path}")
    with open(os.path.join(data_dir, D.SN_FN_FILE), "w") as f:
        f.write("\n".join(lines) + "\n")
    if crop is not None:
        with open(os.path.join(data_dir, D.RESTORE_FILE), "wb") as f:
            pickle.dump({sn: {"pmin": np.array(lo), "pmax": np.array(hi), "shape": tuple(shape)}
                         for sn, (lo, hi) in crop.items()}, f)


def _cube(data_dir, split_dir, **over):
    a = Cf.make_args(Cf.TINY_NET, 4, 4, data_dir=data_dir, split_dir=split_dir, access_type="npy", merge_type=None,
                     patch_size=None)
    for k, v in over.items():
        setattr(a, k, v)
    return D.get_data_cube(a)


def test_sn_fn_and_restore_info_are_read_as_the_reference_reads_them(tmp_path):
    data_dir, split_dir, _ = write_dataset(str(tmp_path), "lits", ["a", "b"], (6, 5, 4))
    assert D.read_restore_info(data_dir) is None
    write_sources(data_dir, ["a"], (9, 8, 7), crop={"a": ((1, 2, 3), (7, 7, 7))})
    with open(os.path.join(data_dir, D.SN_FN_FILE), "a") as f:
        f.write("\nb,/abs/b.nii\n")
    m = D.read_sn_fn(data_dir)
    assert m == {"a": os.path.join(data_dir, "src", "a.nii.gz"), "b": "/abs/b.nii"}
    info = D.read_restore_info(data_dir)
    assert set(info) == {"a"} and tuple(info["a"]["pmax"]) == (7, 7, 7) and info["a"]["shape"] == (9, 8, 7)
    crop = np.arange(120, dtype=np.uint16).reshape(6, 5, 4)
    full = D.restore_crop(crop, **info["a"])
    assert full.shape == (9, 8, 7) and full.dtype == np.uint16 and full.sum() == crop.sum()
    assert np.array_equal(full[1:7, 2:7, 3:7], crop)


def test_src_geom_gives_every_val_subject_its_geometry(tmp_path):
    data_dir, split_dir, _ = write_dataset(str(tmp_path), "lits", ["a", "b", "c"], (6, 5, 4), train=["c"],
                                           val=["b", "a"])
    plain = _cube(data_dir, split_dir)
    assert plain.geometry is None and plain.spacing is None
    write_sources(data_dir, ["a", "b"], (6, 5, 4))
    cube = _cube(data_dir, split_dir, src_geom=True)
    assert cube.val_sn == ["a", "b"] and len(cube.geometry) == 2 and cube.spacing is None
    for e in cube.geometry:
        assert e["spacing"] == (0.7421875, 0.7421875, 5.0) and e["source_shape"] == (6, 5, 4) and "pmin" not in e
        assert np.array_equal(e["affine"][:3], np.array(SRC_ROWS))
    # cropped arrays: the pickle ties them to the source
    write_sources(data_dir, ["a", "b"], (9, 8, 7), crop={"a": ((1, 2, 3), (7, 7, 7)), "b": ((0, 0, 0), (6, 5, 4))})
    cube = _cube(data_dir, split_dir, src_geom=True)
    assert cube.geometry[0]["pmin"] == (1, 2, 3) and cube.geometry[0]["pmax"] == (7, 7, 7)
    assert cube.geometry[1]["source_shape"] == (9, 8, 7)
    sp = _cube(data_dir, split_dir, spacing="5,0.7421875,0.7421875")
    assert sp.geometry is None and sp.spacing == (5.0, 0.7421875, 0.7421875)


def test_every_error_of_src_geom_names_the_subject(tmp_path):
    data_dir, split_dir, _ = write_dataset(str(tmp_path), "lits", ["a", "b"], (6, 5, 4), train=["a"], val=["b"])
    with pytest.raises(RuntimeError, match=r"sn_fn\.txt is missing.*\bb\b"):
        _cube(data_dir, split_dir, src_geom=True)
    write_sources(data_dir, ["a"], (6, 5, 4))
    with pytest.raises(RuntimeError, match="subject b has no line"):
        _cube(data_dir, split_dir, src_geom=True)
    write_sources(data_dir, ["b"], (6, 5, 4))
    open(os.path.join(data_dir, "src", "b.nii.gz"), "wb").write(b"not a nifti file")
    with pytest.raises(RuntimeError, match="subject b: cannot read"):
        _cube(data_dir, split_dir, src_geom=True)
    os.remove(os.path.join(data_dir, "src", "b.nii.gz"))
    with pytest.raises(RuntimeError, match="subject b: cannot read"):
        _cube(data_dir, split_dir, src_geom=True)
    write_sources(data_dir, ["b"], (9, 8, 7))                  # another shape and no pickle
    with pytest.raises(RuntimeError, match=r"subject b: array of shape \(6, 5, 4\), source image of shape \(9, 8, 7\)"):
        _cube(data_dir, split_dir, src_geom=True)
    write_sources(data_dir, ["b"], (9, 8, 7), crop={"b": ((1, 2, 3), (7, 7, 6))})      # pmax - pmin = (6, 5, 3)
    with pytest.raises(RuntimeError, match="subject b: array of shape"):
        _cube(data_dir, split_dir, src_geom=True)
    write_sources(data_dir, ["b"], (9, 8, 7), crop={"b": ((1, 2, 3), (7, 7, 7))})
    assert _cube(data_dir, split_dir, src_geom=True).geometry[0]["pmin"] == (1, 2, 3)
    with pytest.raises(RuntimeError, match="exclude each other"):
        _cube(data_dir, split_dir, src_geom=True, spacing="1,1,1")
    for bad in ("1,1", "0,1,1", "1,-1,1", "1,nan,1", "inf,1,1", "a,b,c"):
        with pytest.raises(RuntimeError, match="--spacing"):
            _cube(data_dir, split_dir, spacing=bad)


def test_parser_knows_the_switches_and_yaml_keys_set_them(tmp_path):
    a = Cf.build_parser().parse_args(["ptq"])
    assert a.src_geom is False and a.spacing is None
    a = Cf.build_parser().parse_args(["ptq", "--src_geom", "--surf_dist"])
    assert a.src_geom is True and a.spacing is None
    assert Cf.build_parser().parse_args(["ptq", "--spacing", "5,0.7,0.7"]).spacing == "5,0.7,0.7"
    m = Cf.make_args(Cf.TINY_NET, 4, 4)
    assert m.src_geom is False and m.spacing is None
    cfg = tmp_path / "g.yaml"
    cfg.write_text("src_geom: true\ntask: lits\n")
    assert Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["ptq"])).src_geom is True
    cfg.write_text("spacing: 5,0.7421875,0.7421875\n")
    args = Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["ptq"]))
    assert D.parse_spacing(args.spacing) == (5.0, 0.7421875, 0.7421875) and args.src_geom is False
    cfg.write_text("spacing: [5, 0.7421875, 0.7421875]\n")
    assert D.parse_spacing(Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["ptq"])).spacing)[0] == 5.0


def test_a_map_is_restored_and_written_with_the_source_geometry(tmp_path):
    data_dir, split_dir, _ = write_dataset(str(tmp_path), "lits", ["a"], (6, 5, 4))
    write_sources(data_dir, ["a"], (9, 8, 7), crop={"a": ((1, 2, 3), (7, 7, 7))})
    entry = _cube(data_dir, split_dir, src_geom=True).geometry[0]
    m = np.arange(120).reshape(6, 5, 4) % 3
    E._write_map(str(tmp_path / "m.nii.gz"), m, np.uint16, entry)
    got, f = N.read_nifti(str(tmp_path / "m.nii.gz"))
    assert got.shape == (9, 8, 7) and got.dtype == np.uint16
    assert np.array_equal(got[1:7, 2:7, 3:7], m) and got.sum() == m.sum()
    g = N.read_geometry(str(tmp_path / "m.nii.gz"))
    src = entry["header"]
    assert np.array_equal(g["affine"], src["affine"]) and g["pixdim"] == src["pixdim"] and g["quatern"] == src["quatern"]
    assert (g["qform_code"], g["sform_code"]) == (1, 1)
    assert g["xyzt_units"] == src["xyzt_units"] == 10
    with pytest.raises(RuntimeError, match="three axes"):      # the planes of --multi_label lits have no source grid
        E._write_map(str(tmp_path / "planes.nii.gz"), np.stack([m, m]), np.uint8, entry)
    E._write_map(str(tmp_path / "plain.nii.gz"), m, np.uint16)
    N.write_nifti(str(tmp_path / "today.nii.gz"), m.astype(np.uint16))
    assert open(tmp_path / "plain.nii.gz", "rb").read() == open(tmp_path / "today.nii.gz", "rb").read()


def test_planes_maps_with_src_geom_stop_the_mission_before_calibration(tmp_path):
    """--multi_label lits writes C x D x H x W planes, which have no place on a source grid: the mission stops with the
    subjects' names before a model is loaded or anything is calibrated."""
    from efficientq_amd import entrance
    data_dir, split_dir, _ = write_dataset(str(tmp_path), "lits", ["a", "b"], (6, 5, 4), train=["a"], val=["b"])
    write_sources(data_dir, ["b"], (6, 5, 4))
    argv = ["ptq", "--task", "lits", "--qconv", "effq", "--qlvl_w", "4", "--qlvl_a", "4", "--q_first", "256,-1",
            "--q_last", "256,-1", "--width", "8,16,8", "--depth", "1,1,1", "--nMod", "1", "--nClass", "3", "--blk", "mid",
            "--ds", "simple", "--hetero_dim", "--multi_label", "lits", "--data_dir", data_dir, "--split_dir", split_dir,
            "--save_nii", "--src_geom", "--snap_dir", str(tmp_path / "snap")]
    with pytest.raises(SystemExit, match=r"one plane per class.*\bb\b"):
        entrance.main(argv)
    assert not os.path.exists(tmp_path / "snap" / "layer_loss.txt")


# ---- surface_metrics_mm and metrics.csv -------------------------------------------------------------------------------
def test_surface_metrics_mm_from_hand_written_values():
    # class 0: n = 21, rank 19 exactly; class 1: n = 4, 95 * 3 = 285: between ranks 2 and 3; class 2: both empty;
    # class 3: one empty -> the physical diagonal of 3 x 4 x 12 voxels of 4 x 3 x 1 mm = 12 sqrt(3)
    counts = torch.tensor([[11, 10], [2, 2], [0, 0], [5, 0]])
    sq = torch.tensor([[49.0, 25.0, 16.0, 36.0], [2.25, 4.0, 4.0, 6.25], [0.0] * 4, [0.0] * 4])
    sums = torch.tensor([[22.0, 10.0], [4.0, 3.0], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64)
    got = E.surface_metrics_mm(counts, sq, sums, (3, 4, 12), (4.0, 3.0, 1.0))
    assert got.dtype == torch.float64 and got.shape == (4, 3)
    assert got[0].tolist() == [7.0, 4.0, 1.5]
    assert got[1].tolist() == [2.0, 2.0 + 0.5 * 85 / 100, (2.0 + 1.5) / 2]
    assert got[2].tolist() == [0.0, 0.0, 0.0]
    assert got[3].tolist() == [math.sqrt(3 * 144.0)] * 3
    assert E.SURFACE_COLUMNS_MM == ("hd_mm", "hd95_mm", "assd_mm") and E.SURFACE_COLUMNS == ("hd", "hd95", "assd")
    # with unit spacing it is surface_metrics on the same numbers
    old = E.surface_metrics(torch.tensor([[11, 10, 49, 25, 16, 36]]), sums[:1], (3, 4, 12))
    assert torch.equal(E.surface_metrics_mm(counts[:1], sq[:1], sums[:1], (3, 4, 12), (1, 1, 1)), old)


def _results(unit):
    res = []
    for name, counts, sd in (("s1", [[3, 1, 2, 4], [1, 0, 0, 9]], [[5.0, 4.25, 1.0 / 3], [0.0, 0.0, 0.0]]),
                             ("s2", [[0, 2, 0, 8], [5, 0, 5, 0]], [[math.sqrt(139225), 373.1286641, 1e-3], [1.0] * 3])):
        r = {"name": name, "counts": torch.tensor(counts)}
        r.update(E.metrics_from_counts(r["counts"]))
        if unit:
            r["surface"] = torch.tensor(sd, dtype=torch.float64)
        if unit == "mm":
            r["surface_unit"] = "mm"
        res.append(r)
    return res


def test_metrics_csv_names_the_columns_by_their_unit(tmp_path):
    plain, vox, mm = (str(tmp_path / n) for n in ("plain.csv", "vox.csv", "mm.csv"))
    E.write_metrics_csv(plain, _results(None))
    E.write_metrics_csv(vox, _results("voxel"))
    E.write_metrics_csv(mm, _results("mm"))
    rows_mm, rows_vox = list(csv.reader(open(mm))), list(csv.reader(open(vox)))
    assert rows_vox[0][10:] == ["hd", "hd95", "assd"] and rows_mm[0][10:] == ["hd_mm", "hd95_mm", "assd_mm"]
    assert rows_mm[1:] == rows_vox[1:] and rows_mm[0][:10] == rows_vox[0][:10]
    stripped = b"".join(b",".join(line.split(b",")[:10]) + b"\r\n" for line in open(mm, "rb").read().splitlines())
    assert stripped == open(plain, "rb").read()
    mixed = _results("mm")
    del mixed[1]["surface_unit"]
    with pytest.raises(RuntimeError):
        E.write_metrics_csv(str(tmp_path / "mixed.csv"), mixed)


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_mm_symbols_in_header_and_signatures():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("effq_surf_mm_ws_bytes", 4), ("effq_edt_sq_mm", 12), ("effq_seg_surface_mm", 18)):
        m = re.search(rf"\b(?:int|size_t) {name}\s*\(([^)]*)\)", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"\bsize_t effq_surf_mm_ws_bytes\s*\(\s*int P, int D, int H, int W\s*\)", hdr)
    assert int(re.search(r"#define EFFQ_EDT_MM_MAX_EXTENT (\d+)", hdr).group(1)) == _lib.EDT_MM_MAX_EXTENT == 4096
    floats = [i for i, t in enumerate(_lib.SIGNATURES["effq_edt_sq_mm"][1]) if t is _lib._F]
    assert floats == [5, 6, 7]
    csrc = os.path.join(ROOT, "efficientq_amd", "csrc")
    text = open(os.path.join(csrc, "seg_surface_mm.hip")).read()
    assert '#include "seg_decide.h"' in text and '#include "seg_masks.h"' in text and "void decide(" not in text
    assert '#include "seg_surf.h"' in text and "void k_surf_bits" not in text
    assert "void k_surf_bits" in open(os.path.join(csrc, "seg_surf.h")).read()
    assert "void k_surf_bits" not in open(os.path.join(csrc, "seg_surface.hip")).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "seg_surface_mm.hip" in mk and "seg_surf.h" in mk and "-ffp-contract=off" in mk
