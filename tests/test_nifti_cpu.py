"""The nibabel-free NIfTI-1 codec of efficientq_amd/nifti.py (no GPU): round trips, the header at the offsets of the
NIfTI-1 specification parsed here with struct, the Fortran-order data block, reproducible .gz bytes, rejections."""
import gzip
import struct

import numpy as np
import pytest

from efficientq_amd.nifti import read_nifti, write_nifti

SHAPES = [(5, 7, 3), (1, 9, 4), (3, 5, 6, 2), (2, 3, 4, 5)]


def _array(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    hi = 5 if dtype == np.uint8 else 60000
    return rng.integers(0, hi, size=shape).astype(dtype)


@pytest.mark.parametrize("suffix", [".nii", ".nii.gz"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", SHAPES)
def test_round_trip(tmp_path, shape, dtype, suffix):
    a = _array(shape, dtype)
    path = str(tmp_path / f"m{suffix}")
    write_nifti(path, a)
    b, hdr = read_nifti(path)
    assert b.dtype == a.dtype and b.shape == a.shape
    assert np.array_equal(a, b)
    assert np.array_equal(hdr["affine"], np.eye(4))


def _raw(path):
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if path.endswith(".gz") else raw


@pytest.mark.parametrize("dtype,code", [(np.uint8, 2), (np.uint16, 512)])
def test_header_fields_at_the_spec_offsets(tmp_path, dtype, code):
    a = _array((6, 4, 3, 2), dtype, seed=1)
    affine = np.array([[2.0, 0, 0, -10], [0, 3.0, 0, 5], [0, 0, 1.5, 7], [0, 0, 0, 1]])
    path = str(tmp_path / "h.nii.gz")
    write_nifti(path, a, affine)
    raw = _raw(path)
    u = lambda fmt, off: struct.unpack_from("<" + fmt, raw, off)
    assert u("i", 0) == (348,)                                     # sizeof_hdr
    assert u("8h", 40) == (4, 6, 4, 3, 2, 1, 1, 1)                 # dim
    assert u("h", 70) == (code,)                                   # datatype
    assert u("h", 72) == (8 * np.dtype(dtype).itemsize,)           # bitpix
    assert u("8f", 76) == (1.0,) * 8                               # pixdim
    assert u("f", 108) == (352.0,)                                 # vox_offset
    assert u("h", 252) == (0,) and u("h", 254) == (2,)             # qform_code, sform_code
    assert u("4f", 280) == tuple(affine[0])                        # srow_x
    assert u("4f", 296) == tuple(affine[1])                        # srow_y
    assert u("4f", 312) == tuple(affine[2])                        # srow_z
    assert raw[344:348] == b"n+1\0"                                # magic
    assert raw[348:352] == b"\0\0\0\0"                             # no extension
    # the data block: little-endian, first array axis fastest
    assert raw[352:] == a.astype(np.dtype(dtype).newbyteorder("<")).tobytes(order="F")
    assert len(raw) == 352 + a.nbytes


def test_same_map_same_bytes(tmp_path):
    a = _array((17, 11, 9), np.uint16, seed=2)
    p1, p2 = str(tmp_path / "a.nii.gz"), str(tmp_path / "b.nii.gz")
    write_nifti(p1, a)
    write_nifti(p2, a.copy(order="F"))
    assert open(p1, "rb").read() == open(p2, "rb").read()


def test_corrupt_magic_size_and_datatype_are_rejected(tmp_path):
    a = _array((4, 4, 4), np.uint8)
    good = str(tmp_path / "g.nii")
    write_nifti(good, a)
    raw = bytearray(open(good, "rb").read())

    def bad(mutate, msg):
        r = bytearray(raw)
        mutate(r)
        path = str(tmp_path / "bad.nii")
        open(path, "wb").write(bytes(r))
        with pytest.raises(ValueError, match=msg):
            read_nifti(path)
    bad(lambda r: r.__setitem__(slice(344, 348), b"ni1\0"), "magic")
    bad(lambda r: struct.pack_into("<i", r, 0, 540), "sizeof_hdr")
    bad(lambda r: struct.pack_into("<h", r, 70, 16), "datatype")
    bad(lambda r: r.__delitem__(slice(400, None)), "does not fit")


def test_writer_rejects_other_dtypes_and_shapes(tmp_path):
    with pytest.raises(ValueError):
        write_nifti(str(tmp_path / "f.nii"), np.zeros((2, 2, 2), np.float32))
    with pytest.raises(ValueError):
        write_nifti(str(tmp_path / "e.nii"), np.zeros((0, 2, 2), np.uint8))
    with pytest.raises(ValueError):
        write_nifti(str(tmp_path / "a.nii"), np.zeros((2, 2, 2), np.uint8), np.eye(3))


def test_nibabel_reads_what_is_written(tmp_path):
    nib = pytest.importorskip("nibabel")
    a = _array((7, 5, 3), np.uint16, seed=3)
    path = str(tmp_path / "n.nii.gz")
    write_nifti(path, a)
    img = nib.load(path)
    assert np.array_equal(np.asanyarray(img.dataobj), a)
    assert np.array_equal(img.affine, np.eye(4))
    assert int(img.header["sform_code"]) == 2 and int(img.header["qform_code"]) == 0
