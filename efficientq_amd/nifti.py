"""Single-file NIfTI-1 (``.nii`` / ``.nii.gz``) label maps without nibabel: what ``--save_nii`` writes.

The writer produces the file ``nib.Nifti1Image(array, affine).to_filename(path)`` describes for an integer label map
(utils/validate.py:247-260, metrics.extract_nii): the 348-byte header, 4 zero extension bytes, the data from byte 352,
``sform_code`` 2 (aligned) with the affine's rows, ``qform_code`` 0, unit ``pixdim``.  The data block is little-endian
and in Fortran order (first array axis fastest), so a NIfTI reader gets back ``array`` with the same axes.  ``.gz``
files carry no name and ``mtime`` 0: the same map always gives the same bytes.

The reader is the inverse for these files (uint8 / uint16 data, either byte order) and rejects anything else.
``read_image`` reads the source scans of the ``prep`` mission: 3-D images of the common integer and float datatypes, as
float32 with the header's scaling applied.

``read_geometry`` reads only the header of an image of any datatype: where the voxels of a scan lie in space.  With
``--src_geom`` the label maps are written with the geometry of the scan they belong to (``write_nifti(..., geometry=)``:
the source's sform and qform fields, codes and ``pixdim``), so that a viewer overlays them, and the surface distances
are measured with the source's spacing.

``BackgroundWriter`` runs the writes of a mission on one background thread while the device goes on.
"""
from __future__ import annotations

import gzip
import struct
import zlib
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HEADER_BYTES = 348
VOX_OFFSET = 352
MAGIC = b"n+1\0"
DATATYPES = {2: np.dtype(np.uint8), 512: np.dtype(np.uint16)}      # NIfTI datatype code -> dtype
_CODES = {v: k for k, v in DATATYPES.items()}
GZIP_LEVEL = 1

# (name, struct format, offset) of the fields used here, NIfTI-1 spec (nifti1.h)
FIELDS = (("sizeof_hdr", "i", 0), ("dim", "8h", 40), ("datatype", "h", 70), ("bitpix", "h", 72),
          ("pixdim", "8f", 76), ("vox_offset", "f", 108), ("scl_slope", "f", 112), ("scl_inter", "f", 116),
          ("xyzt_units", "B", 123),
          ("qform_code", "h", 252), ("sform_code", "h", 254), ("quatern", "6f", 256), ("srow_x", "4f", 280),
          ("srow_y", "4f", 296), ("srow_z", "4f", 312), ("magic", "4s", 344))


def _header(shape, dtype: np.dtype, affine: np.ndarray, geometry=None, scale=None) -> bytes:
    hdr = bytearray(HEADER_BYTES)
    dim = [len(shape)] + list(shape) + [1] * (7 - len(shape))
    values = {"sizeof_hdr": (HEADER_BYTES,), "dim": dim, "datatype": (_CODES[dtype],), "bitpix": (8 * dtype.itemsize,),
              "pixdim": [1.0] * 8, "vox_offset": (float(VOX_OFFSET),), "scl_slope": (0.0,), "scl_inter": (0.0,),
              "xyzt_units": (0,), "qform_code": (0,), "sform_code": (2,), "quatern": [0.0, 0.0, 0.0] + list(affine[:3, 3]),
              "srow_x": list(affine[0]), "srow_y": list(affine[1]), "srow_z": list(affine[2]), "magic": (MAGIC,)}
    if geometry is not None:                                           # the source's own fields, value for value
        values.update({"pixdim": list(geometry["pixdim"]),
                       "xyzt_units": (int(geometry.get("xyzt_units", 0)),), "qform_code": (int(geometry["qform_code"]),),
                       "sform_code": (int(geometry["sform_code"]),), "quatern": list(geometry["quatern"]),
                       "srow_x": list(geometry["srow_x"]), "srow_y": list(geometry["srow_y"]),
                       "srow_z": list(geometry["srow_z"])})
    if scale is not None:                                              # value = scl_slope * stored + scl_inter
        values.update({"scl_slope": (float(scale[0]),), "scl_inter": (float(scale[1]),)})
    for name, fmt, off in FIELDS:
        struct.pack_into("<" + fmt, hdr, off, *values[name])
    hdr[38:39] = b"r"                                                  # `regular`, as the ANALYZE readers expect
    return bytes(hdr)


def encode_nifti(array, affine=None, geometry=None, scale=None) -> bytes:
    """The uncompressed ``.nii`` bytes of a uint8 / uint16 array of 1 to 7 dimensions; see write_nifti."""
    if scale is not None:
        try:
            slope, inter = (float(v) for v in scale)
        except (TypeError, ValueError):
            raise ValueError(f"write_nifti: scale {scale!r}, needs (slope, inter)")
        if not (np.isfinite(slope) and np.isfinite(inter)) or slope == 0.0:
            raise ValueError(f"write_nifti: scale {scale!r}: a finite slope other than 0 and a finite inter")
        scale = (slope, inter)
    a = np.asarray(array)
    if a.dtype.newbyteorder("=") not in _CODES:
        raise ValueError(f"write_nifti: {a.dtype} data, only uint8 and uint16 are written")
    if not 1 <= a.ndim <= 7 or a.size == 0 or max(a.shape) > 32767:
        raise ValueError(f"write_nifti: shape {a.shape} does not fit a NIfTI-1 header")
    aff = np.eye(4) if affine is None else np.asarray(affine, dtype=np.float64)
    if aff.shape != (4, 4):
        raise ValueError(f"write_nifti: affine of shape {aff.shape}, needs 4 x 4")
    if geometry is not None:
        if affine is not None:
            raise ValueError("write_nifti: give an affine or a geometry, not both")
        if tuple(geometry["shape"][:3]) != tuple(a.shape[:3]):
            raise ValueError(f"write_nifti: array of shape {a.shape} for a geometry of shape {tuple(geometry['shape'])}")
    dt = a.dtype.newbyteorder("=")
    data = np.asarray(a, dtype=dt.newbyteorder("<")).tobytes(order="F")
    return _header(a.shape, dt, aff, geometry, scale) + b"\0" * (VOX_OFFSET - HEADER_BYTES) + data


def write_nifti(path: str, array, affine=None, geometry=None, scale=None) -> None:
    """Write `array` (uint8 / uint16) to `path` as a single-file NIfTI-1 image with the given 4 x 4 affine (identity by
    default); a path ending in ``.gz`` is gzip-compressed with no name and mtime 0.  With `geometry` (what read_geometry
    returned for the scan the map belongs to) the header carries that image's sform and qform fields, both codes, its
    ``pixdim`` and its ``xyzt_units`` (what unit the pixdim are in) instead; the other fields of the source header
    (descrip, intent, cal_min / cal_max, slice timing) are not copied.  The array's first three axes are the image's i,
    j, k and must have the source's extents.  With `scale` = (slope, inter) the header's ``scl_slope`` and ``scl_inter``
    are set, so a reader shows ``slope * stored + inter`` (the probability maps of ``predict --save_prob``: 1 / 255 and
    0); without it both are 0, which means no scaling, and the bytes are what they were."""
    raw = encode_nifti(array, affine, geometry, scale)
    with open(path, "wb") as f:
        if str(path).endswith(".gz"):
            with gzip.GzipFile(filename="", mode="wb", compresslevel=GZIP_LEVEL, fileobj=f, mtime=0) as gz:
                gz.write(raw)
        else:
            f.write(raw)


def decode_nifti(raw: bytes):
    """(array, header fields) of the bytes of a single-file NIfTI-1 image; see read_nifti."""
    if len(raw) < VOX_OFFSET:
        raise ValueError(f"read_nifti: {len(raw)} bytes, shorter than a NIfTI-1 header")
    for end in "<>":
        if struct.unpack_from(end + "i", raw, 0)[0] == HEADER_BYTES:
            break
    else:
        raise ValueError(f"read_nifti: sizeof_hdr is not {HEADER_BYTES}: not a NIfTI-1 file")
    f = {}
    for name, fmt, off in FIELDS:
        v = struct.unpack_from(end + fmt, raw, off)
        f[name] = v[0] if len(v) == 1 else v
    if f["magic"] != MAGIC:
        raise ValueError(f"read_nifti: magic {f['magic']!r}, only single-file NIfTI-1 ({MAGIC!r}) is read")
    if f["datatype"] not in DATATYPES:
        raise ValueError(f"read_nifti: datatype {f['datatype']}, only uint8 (2) and uint16 (512) are read")
    dt = DATATYPES[f["datatype"]].newbyteorder(end)
    if f["bitpix"] != 8 * dt.itemsize:
        raise ValueError(f"read_nifti: bitpix {f['bitpix']} for datatype {f['datatype']}")
    ndim = f["dim"][0]
    if not 1 <= ndim <= 7:
        raise ValueError(f"read_nifti: dim[0] = {ndim}")
    shape = tuple(f["dim"][1:1 + ndim])
    off = int(f["vox_offset"])
    n = int(np.prod(shape)) * dt.itemsize
    if min(shape) < 1 or off < VOX_OFFSET or len(raw) < off + n:
        raise ValueError(f"read_nifti: shape {shape} at offset {off} does not fit {len(raw)} bytes")
    a = np.frombuffer(raw, dtype=dt, count=int(np.prod(shape)), offset=off).reshape(shape, order="F")
    f["affine"] = np.array([f["srow_x"], f["srow_y"], f["srow_z"], (0.0, 0.0, 0.0, 1.0)], dtype=np.float64)
    return np.ascontiguousarray(a, dtype=DATATYPES[f["datatype"]]), f


def read_nifti(path: str):
    """(array, header fields) of a single-file NIfTI-1 image of uint8 / uint16 data (gzip-compressed or not).  The
    fields are those of FIELDS plus `affine` (the sform rows); raises ValueError on files of another kind."""
    with open(path, "rb") as fh:
        raw = fh.read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    return decode_nifti(raw)


# ---- geometry --------------------------------------------------------------------------------------------------------
def _read_head(path: str, nbytes: int) -> bytes:
    """The first `nbytes` bytes of a file, or of what a gzip file holds (no more than that is inflated)."""
    with open(path, "rb") as fh:
        head = fh.read(2)
        if head != b"\x1f\x8b":
            return head + fh.read(nbytes - 2)
        z = zlib.decompressobj(wbits=31)
        out, chunk = b"", head + fh.read(1022)
        while chunk and len(out) < nbytes:
            out += z.decompress(chunk, nbytes - len(out))
            while z.unconsumed_tail and len(out) < nbytes:
                out += z.decompress(z.unconsumed_tail, nbytes - len(out))
            chunk = fh.read(1024)
        return out


def qform_affine(quatern, pixdim) -> np.ndarray:
    """The 4 x 4 affine of the qform fields (nifti1.h, "METHOD 2"): quaternion (b, c, d) with a = sqrt(1 - b^2 - c^2 -
    d^2), voxel sizes pixdim[1..3], qfac = -1 when pixdim[0] < 0 (the third column is flipped) and the offsets."""
    b, c, d, qx, qy, qz = (float(v) for v in quatern)
    a2 = 1.0 - (b * b + c * c + d * d)
    a = np.sqrt(a2) if a2 > 0.0 else 0.0
    rot = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                    [2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)],
                    [2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c]], dtype=np.float64)
    qfac = -1.0 if float(pixdim[0]) < 0.0 else 1.0
    aff = np.eye(4)
    aff[:3, :3] = rot * np.array([float(pixdim[1]), float(pixdim[2]), float(pixdim[3]) * qfac])
    aff[:3, 3] = (qx, qy, qz)
    return aff


def _header_fields(raw: bytes, path: str, who: str):
    """(the fields of FIELDS, the byte order) of the header bytes of a single-file NIfTI-1 image, or `who`'s ValueError."""
    for end in "<>":
        if struct.unpack_from(end + "i", raw, 0)[0] == HEADER_BYTES:
            break
    else:
        raise ValueError(f"{who}: {path}: sizeof_hdr is not {HEADER_BYTES}: not a NIfTI-1 file")
    f = {}
    for name, fmt, off in FIELDS:
        v = struct.unpack_from(end + fmt, raw, off)
        f[name] = v[0] if len(v) == 1 else v
    if f["magic"] != MAGIC:
        raise ValueError(f"{who}: {path}: magic {f['magic']!r}, only single-file NIfTI-1 ({MAGIC!r}) is read")
    return f, end


def _affine_and_spacing(f: dict):
    """The affine in the order in which NIfTI readers choose it (read_geometry) and the norms of its first three columns."""
    if f["sform_code"] > 0:
        aff = np.array([f["srow_x"], f["srow_y"], f["srow_z"], (0.0, 0.0, 0.0, 1.0)], dtype=np.float64)
    elif f["qform_code"] > 0:
        aff = qform_affine(f["quatern"], f["pixdim"])
    else:
        aff = np.diag([float(f["pixdim"][1]), float(f["pixdim"][2]), float(f["pixdim"][3]), 1.0])
    return aff, tuple(float(np.sqrt((aff[:3, k] ** 2).sum())) for k in range(3))


def read_geometry(path: str) -> dict:
    """Where the voxels of a single-file NIfTI-1 image (``.nii`` / ``.nii.gz``, either byte order, any datatype) lie,
    from its header alone.  Returns `shape`, `pixdim` (8 values), `qform_code`, `sform_code`, `quatern` (b, c, d and the
    three offsets), `srow_x` / `srow_y` / `srow_z`, `xyzt_units`, `datatype`, and
    affine   the sform rows when sform_code > 0, else the qform (qform_affine) when qform_code > 0, else
             diag(pixdim[1..3]) - the order in which NIfTI readers choose;
    spacing  the Euclidean norm of each of the first three columns of that affine: millimetres per step along array
             axis 0, 1, 2.
    Raises ValueError on anything that is not such a file."""
    raw = _read_head(path, VOX_OFFSET)
    if len(raw) < HEADER_BYTES:
        raise ValueError(f"read_geometry: {path}: {len(raw)} bytes, shorter than a NIfTI-1 header")
    f, _ = _header_fields(raw, path, "read_geometry")
    ndim = f["dim"][0]
    if not 3 <= ndim <= 7 or min(f["dim"][1:1 + ndim]) < 1:
        raise ValueError(f"read_geometry: {path}: dim = {f['dim']}, needs three axes or more")
    g = {k: f[k] for k in ("pixdim", "xyzt_units", "qform_code", "sform_code", "quatern", "srow_x", "srow_y", "srow_z",
                           "datatype")}
    g["shape"] = tuple(int(n) for n in f["dim"][1:1 + ndim])
    g["affine"], g["spacing"] = _affine_and_spacing(f)
    return g


# ---- source scans (the `prep` mission) -----------------------------------------------------------------------------------
# NIfTI datatype code -> dtype of the images read_image reads
IMAGE_DATATYPES = {2: np.dtype(np.uint8), 4: np.dtype(np.int16), 8: np.dtype(np.int32), 16: np.dtype(np.float32),
                   64: np.dtype(np.float64), 256: np.dtype(np.int8), 512: np.dtype(np.uint16), 768: np.dtype(np.uint32)}


def decode_image(raw: bytes, path: str = "<bytes>"):
    """(float32 array, header fields) of the bytes of a single-file NIfTI-1 image; see read_image."""
    if len(raw) < VOX_OFFSET:
        raise ValueError(f"read_image: {path}: {len(raw)} bytes, shorter than a NIfTI-1 header")
    f, end = _header_fields(raw, path, "read_image")
    if f["datatype"] not in IMAGE_DATATYPES:
        raise ValueError(f"read_image: {path}: datatype {f['datatype']}, one of {sorted(IMAGE_DATATYPES)} is read")
    dt = IMAGE_DATATYPES[f["datatype"]].newbyteorder(end)
    if f["bitpix"] != 8 * dt.itemsize:
        raise ValueError(f"read_image: {path}: bitpix {f['bitpix']} for datatype {f['datatype']}")
    ndim = f["dim"][0]
    shape = tuple(int(n) for n in f["dim"][1:1 + max(ndim, 0)])
    if ndim == 4 and shape[3] == 1:                                    # a 4-D image with one volume
        shape = shape[:3]
    if len(shape) != 3 or not 3 <= ndim <= 4 or min(shape) < 1:
        raise ValueError(f"read_image: {path}: dim = {f['dim']}: only 3-D images (or 4-D with a last extent of 1) are read")
    off = int(f["vox_offset"])
    count = int(np.prod(shape))
    if off < VOX_OFFSET or len(raw) < off + count * dt.itemsize:
        raise ValueError(f"read_image: {path}: shape {shape} at offset {off} does not fit {len(raw)} bytes")
    a = np.frombuffer(raw, dtype=dt, count=count, offset=off).reshape(shape, order="F")
    slope, inter = float(f["scl_slope"]), float(f["scl_inter"])
    if slope != 0.0 and np.isfinite(slope) and np.isfinite(inter):     # nifti1.h: scaling applies when scl_slope != 0
        a = (a.astype(np.float64) * slope + inter).astype(np.float32)
    f["affine"], f["spacing"] = _affine_and_spacing(f)
    f["shape"] = shape
    return np.ascontiguousarray(a, dtype=np.float32), f


def read_image(path: str):
    """(float32 array, header fields) of a 3-D single-file NIfTI-1 image (``.nii`` / ``.nii.gz``, either byte order) of
    datatype uint8, int16, int32, float32, float64, int8, uint16 or uint32.  ``value = scl_slope * stored + scl_inter``
    (in float64, then cast) when scl_slope != 0.  Array axes 0, 1, 2 are the image's i, j, k.  A 4-D image whose last
    extent is 1 is squeezed; any other dimensionality, datatype or file kind raises a ValueError naming the path.  The
    fields are those of FIELDS plus `shape`, `affine` and `spacing`, chosen as read_geometry chooses them."""
    with open(path, "rb") as fh:
        raw = fh.read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    return decode_image(raw, str(path))


# ---- writing while the device goes on ------------------------------------------------------------------------------------
class BackgroundWriter:
    """One background thread that runs the writes of a mission in the order they are handed in (validate_seg's maps,
    predict's maps), as a context manager.  `max_pending`: once that many jobs wait, submit first waits for the oldest
    (gzip slower than the device: the host maps do not pile up), and re-raises it when it failed.  On exit every job has
    run and the thread is gone, also when the body raised; the first failed job is re-raised unless the body raised."""

    def __init__(self, thread_name_prefix: str, max_pending=None):
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix=thread_name_prefix)
        self._pending, self._max = deque(), max_pending

    def submit(self, fn, *args):
        while self._max is not None and len(self._pending) >= self._max:
            self._pending.popleft().result()
        job = self._pool.submit(fn, *args)
        self._pending.append(job)
        return job

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self._pool.shutdown(wait=True)
        if exc_type is None:
            for job in self._pending:
                job.result()                    # re-raises a failed write
        return False
