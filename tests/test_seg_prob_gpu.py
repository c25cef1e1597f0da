"""effq_seg_probs_source on a real MI355X (-m gpu): the probability planes and the uncertainty of `predict --save_prob /
--save_unc` against the restatement of tests.seg_prob_ref.

The bar.  The restatement interpolates the logits in fp32 exactly as the kernel does (same operations, one rounding
each), computes p and u from those fp32 values in fp64, and gives the exact real values 255 p and 255 u.  Every stored
byte q must satisfy |q - 255 x| <= 0.5 + E with E = seg_prob_ref.E_PROB = 255 * 16 * 2^-23 (4.9e-4 of a level) for the
probabilities and E_UNC = 255 * 32 * 2^-23 (9.7e-4) for the uncertainty: the fp32 error of the device formulation,
derived in DESIGN section 20 from the operation count with expf and logf within 3 ulp and the division within 2.5 ulp.
No voxel is exempt; a value that is NaN (a NaN logit, or an infinite one met with a weight of 0 in the interpolation)
is stored as 0.  The bound is derived, not measured.  Beside it: the label kernel's decisions against the stored
values, the two store paths, determinism, the argument checks, and the mission end to end with the device ops."""
import ctypes as C

import numpy as np
import pytest
import torch

from efficientq_amd import _lib
from efficientq_amd.hip_ops import _ptr, get_ops
from tests import seg_prob_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["argmax", "sigmoid"]
FINITE = [0.0, 1e-6, -1e-6, 20.0, -20.0, 100.0, -100.0]
NONFINITE = [float("inf"), float("-inf"), float("nan")]
# the geometries of the issue: (source, factors, grid, pmin, box)
TAIL = ((5, 6, 7), None, (5, 6, 7), (0, 0, 0), (5, 6, 7))                             # SW = 7: byte stores
ALIGNED = ((6, 5, 8), None, (6, 5, 8), (0, 0, 0), (6, 5, 8))                          # SW = 8: 4-byte stores
BOXED = ((9, 10, 12), (1.5, 1.4, 2.5), (6, 7, 5), (1, 1, 2), (4, 5, 3))               # outside on every face, past the last
UPSAMPLED = ((5, 6, 7), (1.0, 0.5, 1.0), (5, 12, 7), (0, 2, 0), (5, 9, 7))            # a factor below 1 on one axis
SECOND_TRIP = ((64, 128, 516), None, (64, 128, 516), (0, 0, 0), (64, 128, 516))       # 1056768 row items > 4096 * 256


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def _logits(Cc, box, seed, nonfinite=True):
    """4 N(0, 1) with planted values: each of FINITE (and of NONFINITE) in one channel of one voxel, a voxel whose
    channels are all equal, and a voxel with two equal maxima."""
    g = torch.Generator().manual_seed(seed)
    x = 4.0 * torch.randn((Cc,) + tuple(box), generator=g)
    n = int(np.prod(box))
    flat = x.view(Cc, n)
    plant = FINITE + (NONFINITE if nonfinite else [])
    spots = torch.randperm(n, generator=g)[:len(plant) + 2].tolist()
    for k, (at, val) in enumerate(zip(spots, plant)):
        flat[k % Cc, at] = val
    if len(spots) == len(plant) + 2:
        flat[:, spots[-2]] = 1.25                               # all channels equal
        flat[:, spots[-1]] = flat[:, spots[-1]].max()           # C equal maxima ...
        if Cc > 2:
            flat[0, spots[-1]] -= 3.0                           # ... of which two are left
    return x


def _check(ops, logits, geo, mode, tag, interp=None):
    source, factors, grid, pmin, box = geo
    assert tuple(logits.shape[1:]) == tuple(box)
    P, U, inside, v = R.ref_probs_source(logits.numpy(), pmin, grid, factors, source, mode, interp)
    probs, unc = ops.seg_probs_source(logits.to(DEV), pmin, grid, factors, source, mode, True, True)
    assert probs.dtype == unc.dtype == torch.uint8
    assert tuple(probs.shape) == (logits.shape[0],) + tuple(source) and tuple(unc.shape) == tuple(source)
    probs, unc = probs.cpu().numpy(), unc.cpu().numpy()
    ep = R.check_stored(probs, P, R.E_PROB, f"{tag} probs")
    eu = R.check_stored(unc, U, R.E_UNC, f"{tag} unc")
    print(f"{tag}: {int(inside.sum())} of {inside.size} voxels inside, {int(np.isnan(U).sum())} NaN; largest |q - 255 x|: "
          f"probs {ep:.6f}, unc {eu:.6f}")
    # outside the box: exactly the background
    out = ~inside
    assert not unc[out].any() and not probs[1:, out].any()
    assert (probs[0, out] == (255 if mode == "argmax" else 0)).all()
    return probs, unc, inside, v


# ---- the pointwise bound ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Cc", range(1, 9))
def test_every_class_count_at_the_byte_store_tail(ops, Cc, mode):
    _check(ops, _logits(Cc, TAIL[4], 100 + Cc), TAIL, mode, f"tail C {Cc} {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geo", [BOXED, UPSAMPLED], ids=["boxed", "upsampled"])
def test_boxes_and_factors(ops, geo, mode):
    for Cc in (2, 3, 5):
        _, _, inside, _ = _check(ops, _logits(Cc, geo[4], 200 + Cc), geo, mode, f"{geo[0]} f {geo[1]} C {Cc} {mode}")
        assert 0 < inside.sum() < inside.size
    if geo is BOXED:
        # outside voxels on both faces of d and h and on the low face of w; the box ends with the grid along w, where the
        # last source voxels lie past the last working voxel's centre (t - 0.5 = 4.1 > 4) and belong to it
        for ax in range(2):
            assert not np.moveaxis(inside, ax, 0)[0].any() and not np.moveaxis(inside, ax, 0)[-1].any()
        assert not inside[:, :, 0].any() and inside[:, :, -1].any()
        assert (12 - 0.5) / 2.5 - 0.5 > 5 - 1


def test_four_byte_stores_on_and_off_give_the_same_bytes(ops):
    """SW = 8: an aligned base takes the 4-byte stores, the same output one byte further the byte-wise ones; the bytes
    around either output stay as they were."""
    source, factors, grid, pmin, box = ALIGNED
    n = int(np.prod(source))
    i3, d3 = C.c_int * 3, C.c_double * 3
    for mode, code in (("argmax", _lib.SEG_ARGMAX), ("sigmoid", _lib.SEG_SIGMOID)):
        logits = _logits(3, box, 300)
        P, U, _, _ = R.ref_probs_source(logits.numpy(), pmin, grid, factors, source, mode)
        x = logits.to(DEV)
        got = []
        for off in (0, 1):
            pb = torch.full((3 * n + 16,), 7, dtype=torch.uint8, device=DEV)
            ub = torch.full((n + 16,), 7, dtype=torch.uint8, device=DEV)
            assert pb.data_ptr() % 4 == 0 and ub.data_ptr() % 4 == 0
            pv, uv = pb[8 + off:8 + off + 3 * n], ub[8 + off:8 + off + n]
            rc = ops.lib.effq_seg_probs_source(_ptr(x), 3, i3(*box), i3(*pmin), i3(*grid), d3(1.0, 1.0, 1.0), i3(*source),
                                               code, _ptr(pv), _ptr(uv), ops.stream)
            assert rc == 0
            pb, ub = pb.cpu().numpy(), ub.cpu().numpy()
            for buf, m in ((pb, 3 * n), (ub, n)):
                assert (buf[:8 + off] == 7).all() and (buf[8 + off + m:] == 7).all()
            got.append((pb[8 + off:8 + off + 3 * n].reshape((3,) + source), ub[8 + off:8 + off + n].reshape(source)))
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
        R.check_stored(got[0][0], P, R.E_PROB, f"aligned {mode} probs")
        R.check_stored(got[0][1], U, R.E_UNC, f"aligned {mode} unc")


def test_the_grid_stride_loop_takes_a_second_trip(ops):
    """More row items than 4096 workgroups of 256 threads hold.  One mode: the loop is the same code in both, and the
    fp64 reference of 8.5 million values is what this case costs."""
    source = SECOND_TRIP[0]
    assert source[0] * source[1] * ((source[2] + 3) // 4) > 4096 * 256
    _check(ops, _logits(2, SECOND_TRIP[4], 400), SECOND_TRIP, "argmax", "second trip argmax")


@pytest.mark.parametrize("mode", MODES)
def test_either_output_alone_equals_its_half_of_both_and_two_calls_give_equal_bytes(ops, mode):
    source, factors, grid, pmin, box = BOXED
    x = _logits(4, box, 500).to(DEV)
    both = ops.seg_probs_source(x, pmin, grid, factors, source, mode, True, True)
    again = ops.seg_probs_source(x, pmin, grid, factors, source, mode, True, True)
    assert torch.equal(both[0], again[0]) and torch.equal(both[1], again[1])
    p, none = ops.seg_probs_source(x, pmin, grid, factors, source, mode, True, False)
    assert none is None and torch.equal(p, both[0])
    none, u = ops.seg_probs_source(x, pmin, grid, factors, source, mode, False, True)
    assert none is None and torch.equal(u, both[1])
    p, none = ops.seg_probs_source(x, pmin, grid, factors, source, mode)                 # the defaults: probabilities only
    assert none is None and torch.equal(p, both[0])
    assert int(both[1].max()) > 0 and int(both[0].max()) > 128


# ---- consistency with the label kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", [TAIL, BOXED], ids=["tail", "boxed"])
def test_the_labels_plane_holds_the_largest_stored_probability(ops, geo):
    source, factors, grid, pmin, box = geo
    for Cc in (2, 3, 8):
        logits = _logits(Cc, box, 600 + Cc, nonfinite=False)
        x = logits.to(DEV)
        lab = ops.seg_labels_source(x, pmin, grid, factors, source, "argmax").cpu().numpy()
        probs, _ = ops.seg_probs_source(x, pmin, grid, factors, source, "argmax")
        probs = probs.cpu().numpy()
        at_label = np.take_along_axis(probs, lab[None].astype(np.int64), 0)[0]
        assert (at_label == probs.max(0)).all() and lab.max() > 0, Cc


@pytest.mark.parametrize("geo", [TAIL, BOXED], ids=["tail", "boxed"])
def test_a_decided_channel_stores_its_side_of_one_half(ops, geo):
    """Fuse none, the default threshold: channel c of a voxel is set iff v_c >= thresh, which the label kernel says of the
    channel taken alone (rule rank, one channel: label 1); set stores >= 127, clear <= 128, outside 0."""
    source, factors, grid, pmin, box = geo
    logits = _logits(3, box, 700, nonfinite=False)
    x = logits.to(DEV)
    probs, _ = ops.seg_probs_source(x, pmin, grid, factors, source, "sigmoid")
    probs = probs.cpu().numpy()
    inside = R.ref_logits_source(logits.numpy(), pmin, grid, factors, source)[1]
    for c in range(3):
        bit = ops.seg_labels_source(x[c:c + 1].contiguous(), pmin, grid, factors, source, "rank").cpu().numpy()
        assert set(np.unique(bit)) == {0, 1}
        assert (probs[c][bit == 1] >= 127).all() and (probs[c][(bit == 0) & inside] <= 128).all()
        assert not probs[c][~inside].any()


# ---- arguments ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(ops):
    x = torch.randn(3, 4, 5, 6, device=DEV)
    ok = ((0, 0, 0), (4, 5, 6), (1.0, 1.0, 1.0), (4, 5, 6))
    p, u = ops.seg_probs_source(x, *ok, "argmax", True, True)
    assert p.shape == (3, 4, 5, 6) and u.shape == (4, 5, 6)
    with pytest.raises(_lib.EffqError):
        ops.seg_probs_source(x, *ok, "argmax", False, False)                              # nothing wanted
    with pytest.raises(_lib.EffqError):
        ops.seg_probs_source(x, *ok, "softmax")                                           # no such mode
    with pytest.raises(_lib.EffqError):
        ops.seg_probs_source(torch.randn(9, 4, 5, 6, device=DEV), *ok, "sigmoid")         # the class limit
    with pytest.raises(_lib.EffqError):
        ops.seg_probs_source(x, (1, 0, 0), (4, 5, 6), (1.0, 1.0, 1.0), (4, 5, 6), "argmax")      # pmin + g > G
    with pytest.raises(_lib.EffqError):
        ops.seg_probs_source(x, (0, 0, 0), (4, 5, 6), (1.0, float("nan"), 1.0), (4, 5, 6), "argmax")
    with pytest.raises(_lib.EffqError):
        ops.seg_probs_source(x, *ok[:3], (1024, 1024, 1024), "argmax")                    # 3 * 2^30 bytes of planes
    with pytest.raises(_lib.EffqError):
        ops.seg_probs_source(x, *ok[:3], (2048, 2048, 512), "argmax", False, True)        # 2^31 voxels
    # the entry point itself, past the wrapper's own checks
    i3, d3, ERR_ARG = C.c_int * 3, C.c_double * 3, 1            # include/effq_hip.h: EFFQ_ERR_ARG
    out = torch.full((3 * 4 * 5 * 6,), 9, dtype=torch.uint8, device=DEV)

    def raw(Cc=3, pmin=(0, 0, 0), f=(1.0, 1.0, 1.0), source=(4, 5, 6), mode=0, probs=out, unc=out, logits=x):
        return ops.lib.effq_seg_probs_source(_ptr(logits), Cc, i3(4, 5, 6), i3(*pmin), i3(4, 5, 6), d3(*f), i3(*source),
                                             mode, _ptr(probs), _ptr(unc), ops.stream)
    assert raw(probs=None, unc=None) == ERR_ARG                 # both outputs null
    assert raw(Cc=9) == ERR_ARG and raw(Cc=0) == ERR_ARG
    assert raw(pmin=(0, 1, 0)) == ERR_ARG and raw(pmin=(-1, 0, 0)) == ERR_ARG
    assert raw(f=(1.0, 1.0, float("nan"))) == ERR_ARG and raw(f=(0.0, 1.0, 1.0)) == ERR_ARG
    assert raw(source=(2048, 2048, 512)) == ERR_ARG              # 2^31 voxels by shape alone
    assert raw(source=(1024, 1024, 1024), Cc=2) == ERR_ARG       # C * voxels = 2^31 with the planes wanted
    assert raw(source=(4, 40000, 6)) == ERR_ARG and raw(mode=2) == ERR_ARG and raw(logits=None) == ERR_ARG
    torch.cuda.synchronize()                                     # nothing faulted on the way
    assert (out == 9).all()                                      # and nothing was launched


# ---- the mission end to end -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_mission_end_to_end_on_a_turned_and_resampled_scan(ops, tmp_path, mode):
    """predict --save_prob --save_unc --prep_orient --prep_spacing with the device ops on a scan stored in another
    orientation: the files hold what one call of seg_probs_source gives for the mission's own logits, put back on the
    scan's axes; they meet the bar of this module against the restatement; the label map and the table do not change."""
    import os

    from efficientq_amd import evaluate as E, nifti, predict, prep
    from tests.test_orient_cpu import CANON, VARIANTS, ref_reorient, variant_affine
    from tests.test_predict_cpu import PointNet, ct_like, predict_args
    from tests.test_prep_cpu import write_scan
    root = str(tmp_path)
    turned = VARIANTS[4]
    vol, _ = ct_like(3)
    os.makedirs(os.path.join(root, "src"))
    write_scan(os.path.join(root, "src", "t.nii.gz"), ref_reorient(vol, *turned),
               affine=variant_affine(CANON, *turned, vol.shape))
    lst = os.path.join(root, "cases.csv")
    with open(lst, "w") as f:
        f.write("subject,ct\nt,src/t.nii.gz\n")
    kw = dict(src_list=lst, patch_size="8,8,8", prep_mask="nonzero", prep_orient="RAS", prep_spacing="2,1.5,2.5")
    if mode == "sigmoid":
        kw.update(multi_label="brats", merge_type="con")
    model = PointNet().to(DEV)
    predict.run(predict_args(out_dir=os.path.join(root, "plain"), **kw), model=model, window_batch=8)
    predict.run(predict_args("--save_prob", "--save_unc", out_dir=os.path.join(root, "both"), **kw), model=model,
                window_batch=8)
    for name in ("t.nii.gz", "predict.csv"):
        assert open(os.path.join(root, "plain", name), "rb").read() == open(os.path.join(root, "both", name), "rb").read()
    assert sorted(os.listdir(os.path.join(root, "plain"))) == ["predict.csv", "t.nii.gz"]
    entry = prep.read_src_list(lst, "lits")[0]
    plan = prep._Plan(dict(entry, seg=None), ("ct",), (2.0, 1.5, 2.5), (8, 8, 8), "RAS")
    imgs = {"ct": nifti.read_image(entry["images"]["ct"])[0]}
    y, _, _, pmin, _, _, _, _ = prep.process_subject(ops, plan, imgs, None, ("ct",), prep.PrepOptions(
        "nonzero", (-200.0, 250.0), (2.0, 1.5, 2.5), (8, 8, 8), False, "RAS"))
    outs, _, _ = E.stitched_window_logits(ops, [model], torch.from_numpy(y)[None].to(DEV), (8, 8, 8), (4, 4, 4), 8)
    logits = outs[0][0]
    probs, unc = ops.seg_probs_source(logits, pmin, plan.grid_shape, plan.factors, plan.oriented_shape, mode, True, True)
    P, U, inside, _ = R.ref_probs_source(logits.cpu().numpy(), pmin, plan.grid_shape, plan.factors, plan.oriented_shape,
                                         mode)
    R.check_stored(probs.cpu().numpy(), P, R.E_PROB, f"mission {mode} probs")
    R.check_stored(unc.cpu().numpy(), U, R.E_UNC, f"mission {mode} unc")
    assert 0 < inside.sum() < inside.size and tuple(plan.factors) != (1.0, 1.0, 1.0)
    back = prep.orient_inverse(*plan.orient)
    got_p, hp = nifti.read_nifti(os.path.join(root, "both", "prob", "t.nii.gz"))
    got_u, hu = nifti.read_nifti(os.path.join(root, "both", "unc", "t.nii.gz"))
    scan = nifti.read_geometry(entry["images"]["ct"])
    assert got_p.shape == tuple(scan["shape"]) + (3,) and got_u.shape == tuple(scan["shape"]) == (28, 20, 24)
    assert np.array_equal(got_p, np.moveaxis(ref_reorient(probs.cpu().numpy(), *back), 0, -1))
    assert np.array_equal(got_u, ref_reorient(unc.cpu().numpy(), *back))
    for h in (hp, hu):
        assert np.array_equal(h["affine"], scan["affine"]) and h["scl_slope"] == np.float32(1 / 255) and h["scl_inter"] == 0
    assert got_u.max() > 128 and len(np.unique(got_p)) > 50
