"""effq_prep_reorient on a real MI355X (-m gpu): both variants bit for bit against numpy.flip(numpy.transpose(...))
(test_orient_cpu.ref_reorient) over all 48 orientations, over shapes that cross the tiles (64 words for fp32, 128 bytes
for uint8), the 16-B vectors and their tails, with uint8 volumes that start 1 and 3 bytes into a larger buffer on either
side (handled, as the header comment of csrc/reorient.hip says); the plan query; determinism; the argument checks; and the
`prep` and `predict` missions with --prep_orient on a scan stored with its slice axis first and two axes reversed.  A
permutation has no tolerance: everything is compared as integers."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, data as D, nifti, predict, prep
from efficientq_amd.hip_ops import get_ops
from tests.test_orient_cpu import VARIANTS, _write_ct_variants, _write_variant, ref_reorient
from tests.test_predict_cpu import PointNet, predict_args
from tests.test_prep_cpu import prep_args, write_list

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PERMS = list(itertools.permutations(range(3)))
FLIPS = list(itertools.product((False, True), repeat=3))
ERR_ARG = 1                                                     # include/effq_hip.h: EFFQ_ERR_ARG


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def _volumes(shape, dtype, seed):
    """Random bits: the float32 ones hold NaNs with payloads, both zeros, infinities and denormals among the rest."""
    g = np.random.default_rng(seed)
    if dtype == np.uint8:
        return g.integers(0, 256, size=shape, dtype=np.uint8)
    bits = g.integers(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64).astype(np.int32)
    flat = bits.reshape(-1)
    special = np.array([0x7fc00001, 0x7f800001, -0x3fffff, 0x7fffffff, 0, -2 ** 31, 0x7f800000, -0x800000, 1],
                       dtype=np.int64).astype(np.int32)       # quiet and signalling NaNs, +-0, +-inf, a denormal
    flat[:special.size] = special[:flat.size]
    return bits.view(np.float32)


def _ints(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _variant_of(perm):
    return 0 if perm[2] == 2 else 1


def _check(ops, x, perm, flip, tag):
    eb = x.dtype.itemsize
    assert ops.prep_reorient_variant(perm, flip, eb) == _variant_of(perm), tag
    got = ops.prep_reorient(torch.from_numpy(x).to(DEV), perm, flip)
    want = ref_reorient(x, perm, flip)
    assert tuple(got.shape) == want.shape and got.is_contiguous(), tag
    assert np.array_equal(_ints(got.cpu().numpy()), _ints(want)), tag


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("shape", [(5, 7, 9), (3, 33, 66)])
def test_all_48_orientations_bit_for_bit(ops, shape, dtype):
    for N in (1, 3):
        x = _volumes((N,) + shape, dtype, 10 * N + len(shape) + shape[2])
        if dtype == np.float32:
            assert np.isnan(x).sum() >= 3 and np.isinf(x).sum() >= 2
        for perm in PERMS:
            for flip in FLIPS:
                _check(ops, x, perm, flip, f"N {N} {shape} {np.dtype(dtype).name} perm {perm} flip {flip}")
    # a plain D x H x W tensor is taken too
    x = _volumes(shape, dtype, 5)
    got = ops.prep_reorient(torch.from_numpy(x).to(DEV), (2, 0, 1), (True, False, True))
    assert np.array_equal(_ints(got.cpu().numpy()), _ints(ref_reorient(x, (2, 0, 1), (True, False, True))))


EDGE_SHAPES = [(33, 31, 65), (64, 64, 64), (1, 70, 3), (129, 2, 34)]
EDGE_FLIPS = [(False, False, False), (True, True, True), (True, False, True)]      # masks 0, 7 and 5


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_permutations_and_flips_across_tile_edges_and_tails(ops, shape, dtype):
    x = _volumes((2,) + shape, dtype, sum(shape))
    for perm in PERMS:
        for flip in EDGE_FLIPS:
            _check(ops, x, perm, flip, f"{shape} {np.dtype(dtype).name} perm {perm} flip {flip}")


def _raw(ops, x_ptr, dims, axes, mask, eb, y_ptr):
    cax = None if axes is None else (C.c_int * 3)(*axes)
    return ops.lib.effq_prep_reorient(C.c_void_p(x_ptr) if x_ptr else None, *dims, cax, mask, eb,
                                      C.c_void_p(y_ptr) if y_ptr else None, ops.stream)


@pytest.mark.parametrize("shape", EDGE_SHAPES)
@pytest.mark.parametrize("off", [(1, 0), (3, 0), (0, 3), (1, 3), (3, 1)])
def test_uint8_volumes_that_start_at_any_byte_are_handled(ops, shape, off):
    """Source and destination 1 and 3 bytes into a larger buffer; the bytes around the destination stay as they were."""
    n = 2 * int(np.prod(shape))
    x = _volumes((2,) + shape, np.uint8, 7 + off[0])
    src = torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
    src[off[0]:off[0] + n] = torch.from_numpy(x).reshape(-1).to(DEV)
    xs = src[off[0]:off[0] + n].view((2,) + shape)
    assert xs.data_ptr() % 4 == off[0] % 4 and xs.is_contiguous()
    for perm in PERMS:
        for flip in EDGE_FLIPS:
            want = ref_reorient(x, perm, flip)
            mask = sum(1 << p for p in range(3) if flip[p])
            tag = f"{shape} off {off} perm {perm} flip {flip}"
            if off[1] == 0:                                     # through the op: the slice goes in as it is
                got = ops.prep_reorient(xs, perm, flip).cpu().numpy()
            else:
                dst = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device=DEV)
                assert dst.data_ptr() % 4 == 0
                rc = _raw(ops, xs.data_ptr(), (2,) + shape, perm, mask, 1, dst.data_ptr() + off[1])
                assert rc == 0, tag
                host = dst.cpu().numpy()
                assert (host[:off[1]] == 0xA5).all() and (host[off[1] + n:] == 0xA5).all(), tag
                got = host[off[1]:off[1] + n].reshape(want.shape)
            assert np.array_equal(got, want), tag


def test_plan_query_reports_the_row_variant_exactly_when_w_stays_innermost(ops):
    for eb in (1, 4):
        for perm in PERMS:
            for flip in FLIPS:
                assert ops.prep_reorient_variant(perm, flip, eb) == (0 if perm[2] == 2 else 1)
    assert sum(_variant_of(p) == 0 for p in PERMS) == 2
    v = C.c_int(-7)
    ax = (C.c_int * 3)(0, 1, 2)
    plan = ops.lib.effq_prep_reorient_plan
    assert plan(ax, 0, 4, C.byref(v)) == 0 and v.value == 0
    assert plan((C.c_int * 3)(0, 0, 2), 0, 4, C.byref(v)) == ERR_ARG
    assert plan((C.c_int * 3)(0, 1, 3), 0, 4, C.byref(v)) == ERR_ARG
    assert plan(ax, 8, 4, C.byref(v)) == ERR_ARG and plan(ax, -1, 4, C.byref(v)) == ERR_ARG
    assert plan(ax, 0, 2, C.byref(v)) == ERR_ARG and plan(None, 0, 4, C.byref(v)) == ERR_ARG
    assert plan(ax, 0, 4, None) == ERR_ARG and v.value == 0


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_two_calls_give_equal_bits(ops, dtype):
    x = torch.from_numpy(_volumes((2, 33, 31, 65), dtype, 3)).to(DEV)
    for perm, flip in (((0, 1, 2), (False, False, True)), ((2, 1, 0), (True, False, True)), ((1, 2, 0), (False, True, False))):
        a, b = ops.prep_reorient(x, perm, flip), ops.prep_reorient(x, perm, flip)
        assert a.data_ptr() != b.data_ptr() and np.array_equal(_ints(a.cpu().numpy()), _ints(b.cpu().numpy()))


def test_every_argument_check_refuses_before_any_launch(ops):
    x = torch.arange(4 * 5 * 6 * 2, dtype=torch.float32, device=DEV).reshape(2, 4, 5, 6)
    y = torch.full((2 * 4 * 5 * 6,), -1.0, dtype=torch.float32, device=DEV)
    dims, ax = (2, 4, 5, 6), (1, 2, 0)
    px, py = x.data_ptr(), y.data_ptr()
    assert _raw(ops, px, dims, ax, 5, 4, py) == 0
    torch.cuda.synchronize()
    want = y.clone()
    assert np.array_equal(want.cpu().numpy().reshape(2, 5, 6, 4), ref_reorient(x.cpu().numpy(), ax, (True, False, True)))
    assert _raw(ops, px, dims, (0, 0, 2), 0, 4, py) == ERR_ARG                    # no permutation
    assert _raw(ops, px, dims, (0, 1, 3), 0, 4, py) == ERR_ARG and _raw(ops, px, dims, (-1, 1, 2), 0, 4, py) == ERR_ARG
    assert _raw(ops, px, dims, ax, 8, 4, py) == ERR_ARG and _raw(ops, px, dims, ax, -1, 4, py) == ERR_ARG
    assert _raw(ops, px, dims, ax, 0, 2, py) == ERR_ARG and _raw(ops, px, dims, ax, 0, 8, py) == ERR_ARG
    assert _raw(ops, px, (1, 32768, 1, 1), ax, 0, 4, py) == ERR_ARG               # an extent of 32768
    assert _raw(ops, px, (1, 1, 1, 32768), ax, 0, 1, py) == ERR_ARG and _raw(ops, px, (2, 0, 5, 6), ax, 0, 4, py) == ERR_ARG
    assert _raw(ops, px, (1 << 16, 32, 32, 32), ax, 0, 1, py) == ERR_ARG           # N D H W = 2^31
    assert _raw(ops, 0, dims, ax, 0, 4, py) == ERR_ARG and _raw(ops, px, dims, ax, 0, 4, 0) == ERR_ARG
    assert _raw(ops, px, dims, None, 0, 4, py) == ERR_ARG                          # null pointers
    assert _raw(ops, px, dims, ax, 0, 4, px) == ERR_ARG                            # y is x
    assert _raw(ops, px, (1, 4, 5, 6), ax, 0, 4, px + 4 * 119) == ERR_ARG          # y begins in the last word of x
    assert _raw(ops, px + 4 * 119, (1, 4, 5, 6), ax, 0, 4, px) == ERR_ARG          # x begins in the last word of y
    assert _raw(ops, px, (1, 4, 5, 6), ax, 0, 4, px + 4 * 120) == 0                # side by side is no overlap
    assert _raw(ops, px + 2, (1, 4, 5, 6), ax, 0, 4, py) == ERR_ARG                # fp32 needs 4-B alignment
    assert _raw(ops, px, (1, 4, 5, 6), ax, 0, 4, py + 1) == ERR_ARG
    torch.cuda.synchronize()                                                       # nothing faulted on the way
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))               # and nothing was written
    with pytest.raises(_lib.EffqError):
        ops.prep_reorient(x, (0, 1, 1), (False, False, False))
    with pytest.raises(_lib.EffqError):
        ops.prep_reorient(x.double(), (0, 1, 2), (False, False, False))
    with pytest.raises(_lib.EffqError):
        ops.prep_reorient(x.transpose(2, 3), (0, 1, 2), (False, False, False))    # not contiguous
    with pytest.raises(_lib.EffqError):
        ops.prep_reorient(x, (0, 1, 2), (False, False))


# ---- the missions on the device -------------------------------------------------------------------------------------------
TURNED = VARIANTS[4]            # the slice axis first, two axes reversed: the tiled variant with flips


def test_prep_of_a_turned_scan_equals_prep_of_the_canonical_scan_byte_for_byte(ops, tmp_path):
    assert TURNED == ((2, 0, 1), (True, True, False))
    root = str(tmp_path)
    rows = [_write_variant(root, "canon", 21, VARIANTS[0])[0], _write_variant(root, "turned", 21, TURNED)[0]]
    kw = dict(prep_min_size="6,6,6", prep_spacing="2,1.5,2")
    plain, out = os.path.join(root, "plain"), os.path.join(root, "out")
    prep.run(prep_args(src_list=write_list(tmp_path / "canon.csv", rows[:1]), data_dir=plain, **kw))
    prep.run(prep_args(src_list=write_list(tmp_path / "both.csv", rows), data_dir=out, prep_orient="RAS", **kw))
    for sn in ("canon", "turned"):
        for m in D.MODALITIES["brats"] + ("seg",):
            a = open(os.path.join(out, m, f"{sn}.npy"), "rb").read()
            assert a == open(os.path.join(plain, m, "canon.npy"), "rb").read() and len(a) > 128, (sn, m)
    flair = np.load(os.path.join(out, "flair", "turned.npy"))
    assert flair.std() > 0.5 and np.array_equal(nifti.read_nifti(os.path.join(out, "grid", "turned.nii.gz"))[0],
                                                nifti.read_nifti(os.path.join(plain, "grid", "canon.nii.gz"))[0])


def test_predict_of_a_turned_scan_is_the_turned_map_of_the_canonical_scan(ops, tmp_path):
    root = str(tmp_path)
    lst, canon, _ = _write_ct_variants(root, 9)
    kw = dict(patch_size="8,8,8", prep_mask="nonzero")
    plain, out = os.path.join(root, "plain"), os.path.join(root, "seg")
    predict.run(predict_args(src_list=canon, out_dir=plain, **kw), model=PointNet(), window_batch=3)
    want, _ = nifti.read_nifti(os.path.join(plain, "v0.nii.gz"))
    assert len(np.unique(want)) == 3
    predict.run(predict_args(src_list=lst, out_dir=out, prep_orient="RAS", **kw), model=PointNet(), window_batch=3)
    for i, (src, flip) in enumerate(VARIANTS):
        got, h = nifti.read_nifti(os.path.join(out, f"v{i}.nii.gz"))
        scan = nifti.read_geometry(os.path.join(root, "src", f"v{i}.nii.gz"))
        assert got.shape == tuple(scan["shape"]) and np.array_equal(h["affine"], scan["affine"])
        assert np.array_equal(got, ref_reorient(want, src, flip)), i
