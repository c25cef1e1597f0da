"""The `prep` kernels (csrc/prep.hip) against the numpy fp64 restatement of tests/test_prep_cpu.py, and the mission end to
end on the device: scans in, the arrays and index files of the `ptq` mission out, and validate_seg writing its maps back
onto the source scans.  Every bound is derived from the arithmetic (see each test), none is measured."""
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, data as D, entrance, evaluate as E, nifti, prep
from efficientq_amd.hip_ops import get_ops
from tests import test_prep_cpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRIDS = [(1, 1, 1), (19, 23, 37), (64, 64, 65)]     # one voxel; no extent a multiple of 4 or 256; 260 workgroups
U53, U24 = 2.0 ** -53, 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def masks_for(grid):
    """name -> boolean union pattern (D, H, W); on the one-voxel grid the patterns that need room collapse to it."""
    d, h, w = grid
    out = {"faces": np.zeros(grid, bool), "single": np.zeros(grid, bool), "blobs": np.zeros(grid, bool)}
    f = out["faces"]
    f[0, h // 2, w // 2] = f[d - 1, h // 3, w // 3] = f[d // 2, 0, w // 2] = f[d // 3, h - 1, w // 3] = True
    f[d // 2, h // 2, 0] = f[d // 3, h // 3, w - 1] = True
    out["single"][d // 2, h // 2, (w // 2) | (1 if w > 1 else 0)] = True
    b = out["blobs"]
    b[d // 8:d // 8 + max(1, d // 5), h // 2:h // 2 + max(1, h // 4), w // 8:w // 8 + max(1, w // 6)] = True
    b[d // 2:d // 2 + max(1, d // 4), h // 8:h // 8 + max(1, h // 5), w // 2 + 1:w // 2 + 1 + max(1, w // 3)] = True
    return out


def subject(grid, C, pattern, seed, empty_modality=None):
    """C modalities, non-zero (mean 3000, std 2: CT-like) inside `pattern` thinned per modality, exactly zero outside."""
    g = np.random.default_rng(seed)
    x = np.zeros((C,) + grid, dtype=np.float32)
    for c in range(C):
        keep = pattern & ((g.random(grid) < 0.8) | (c == 0))          # modality 0 carries the whole pattern
        v = (3000.0 + 2.0 * g.standard_normal(grid)).astype(np.float32)
        x[c] = np.where(keep, v, np.float32(0))
    if empty_modality is not None:
        x[empty_modality] = 0
    return x


def check_moments(ops, x, mask):
    box, count, total = R.ref_bbox_moments(x, mask)
    b1, n1, s1 = ops.prep_bbox_moments(dev(x), mask)
    b2, n2, s2 = ops.prep_bbox_moments(dev(x), mask)
    assert b1.cpu().tolist() == box and n1.cpu().tolist() == count
    m = R.ref_mask(x, mask)
    for c in range(x.shape[0]):
        # any order of adding n fp64 terms is within n 2^-53 sum |x| of the sum
        bound = count[c] * U53 * float(np.abs(x[c][m[c]].astype(np.float64)).sum())
        print(f"moments C={x.shape[0]} grid={x.shape[1:]} c={c}: |diff| = {abs(s1[c].item() - total[c]):.3e} bound = {bound:.3e}")
        assert abs(s1[c].item() - total[c]) <= bound
    assert torch.equal(b1, b2) and torch.equal(n1, n2) and torch.equal(s1.view(torch.int64), s2.view(torch.int64))
    return box, count, total


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("C", [1, 4])
def test_bbox_moments_equal_numpy(ops, grid, C):
    for k, (name, pattern) in enumerate(masks_for(grid).items()):
        box, count, _ = check_moments(ops, subject(grid, C, pattern, 10 + k), "nonzero")
        idx = np.nonzero(pattern)
        assert box == [int(i.min()) for i in idx] + [int(i.max()) for i in idx], name
    if C > 1:                                                          # one modality zero everywhere, another not
        box, count, _ = check_moments(ops, subject(grid, C, masks_for(grid)["blobs"], 20, empty_modality=1), "nonzero")
        assert count[1] == 0 and count[0] > 0
    box, count, _ = check_moments(ops, np.zeros((C,) + grid, np.float32), "nonzero")       # nothing anywhere
    assert box == list(grid) + [-1, -1, -1] and all(a > b for a, b in zip(box[:3], box[3:])) and count == [0] * C
    dense = (3000.0 + 2.0 * np.random.default_rng(3).standard_normal((C,) + grid)).astype(np.float32)
    dense[:, 0, 0, 0] = 0                                              # `all` counts a zero voxel too
    box, count, _ = check_moments(ops, dense, "all")
    assert box == [0, 0, 0] + [n - 1 for n in grid] and count == [int(np.prod(grid))] * C
    check_moments(ops, dense, "nonzero")


def crop_boxes(grid):
    d, h, w = grid
    boxes = [((0, 0, 0), grid), ((d // 2, 0, 0), (d // 2 + 1, h, w))]                    # the grid; one voxel thick
    if w >= 9:
        boxes += [((1, 2, 3), (d - 1, h - 3, w - 2)), ((0, 1, 5), (d, h, w - 1)),        # odd offsets on the fast axis
                  ((d // 3, h // 3, 1), (d // 3 + 2, h // 3 + 1, 2))]                    # one voxel wide
    return boxes


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("mask", ["nonzero", "all"])
def test_sqdev_and_standardise_crop_on_ct_like_data(ops, grid, C, mask):
    if grid == (1, 1, 1):
        x = np.full((C, 1, 1, 1), 3000.5, np.float32)
    else:
        x = subject(grid, C, np.random.default_rng(1).random(grid) < 0.7, 5)
        x[:, 0, 0, 0] = 0
    m = R.ref_mask(x, mask)
    _, count, total = R.ref_bbox_moments(x, mask)
    mean = [s / n for s, n in zip(total, count)]
    sq_ref = R.ref_sqdev(x, mean, mask)
    sq = ops.prep_sqdev(dev(x), mean, mask)
    assert torch.equal(sq.view(torch.int64), ops.prep_sqdev(dev(x), mean, mask).view(torch.int64))
    std_ref = []
    for c in range(C):
        n = count[c]
        got, want = float(np.sqrt(sq[c].item() / n)), float(np.sqrt(sq_ref[c] / n))
        # each term (x - mean)^2 carries two roundings and a sum of n terms n more: (n + 2) 2^-53 relative on either
        # side; the square root halves the sum of both and, with the division, adds two roundings on either side
        bound = want * ((n + 2) * U53 + 4 * U53)
        print(f"std grid={grid} C={C} {mask} c={c}: {got!r} vs {want!r}, bound {bound:.3e}")
        assert abs(got - want) <= bound
        std_ref.append(want if want > 0 else 1.0)
    for pmin, pmax in crop_boxes(grid):
        want = R.ref_standardise_crop(x, pmin, pmax, mean, std_ref, mask)
        got = ops.prep_standardise_crop(dev(x), pmin, pmax, mean, std_ref, mask).cpu().numpy()
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))), (pmin, pmax)
        bg = ~m[:, pmin[0]:pmax[0], pmin[1]:pmax[1], pmin[2]:pmax[2]]
        assert np.all(got.view(np.uint32)[bg] == 0)                    # +0.0f, bit for bit
    lab = np.random.default_rng(2).integers(0, 256, size=(1,) + grid).astype(np.uint8)
    for pmin, pmax in crop_boxes(grid):
        got = ops.prep_crop_u8(dev(lab), pmin, pmax).cpu().numpy()
        assert np.array_equal(got, lab[:, pmin[0]:pmax[0], pmin[1]:pmax[1], pmin[2]:pmax[2]])
    assert np.array_equal(ops.prep_union_mask(dev(x), mask).cpu().numpy(), m.any(0).astype(np.uint8))


def test_prep_arguments_are_checked_before_any_launch(ops):
    x = torch.zeros(1, 4, 5, 6, device=DEV)
    for pmin, pmax in (((0, 0, 0), (4, 5, 7)), ((-1, 0, 0), (4, 5, 6)), ((2, 0, 0), (2, 5, 6))):
        with pytest.raises(_lib.EffqError):
            ops.prep_standardise_crop(x, pmin, pmax, [0.0], [1.0])
        with pytest.raises(_lib.EffqError):
            ops.prep_crop_u8(x.to(torch.uint8), pmin, pmax)
    with pytest.raises(_lib.EffqError):
        ops.prep_bbox_moments(torch.zeros(5, 4, 5, 6, device=DEV))       # more modalities than the kernels take
    with pytest.raises(_lib.EffqError):
        ops.prep_bbox_moments(x, "body")
    with pytest.raises(_lib.EffqError):
        ops.prep_resample(x, (1.0, 0.0, 1.0), (4, 5, 6))
    with pytest.raises(_lib.EffqError):
        ops.prep_window(x, 2.0, 1.0)


@pytest.mark.parametrize("n", [1, 7, 4 * 256 * 3 + 5])
def test_window_equals_numpy_clip(ops, n):
    g = np.random.default_rng(n)
    x = (300.0 * g.standard_normal(n)).astype(np.float32)
    x[::5] = np.resize(np.array([-200.0, 250.0, np.inf, -np.inf, 250.00002], np.float32), len(x[::5]))
    want = np.clip(x, np.float32(-200.0), np.float32(250.0))
    t = dev(x)
    assert ops.prep_window(t, -200.0, 250.0) is t
    assert np.array_equal(t.cpu().numpy(), want)
    off = dev(np.concatenate([np.zeros(1, np.float32), x]))[1:]           # 4-B aligned only
    ops.prep_window(off, -200.0, 250.0)
    assert np.array_equal(off.cpu().numpy(), want)


FACTORS = [(1.0, 1.0, 1.0), (0.5, 0.75, 2.5), (3.0, 1.0, 0.4), (40.0, 0.5, 100.0)]    # the last: extents of 1


@pytest.mark.parametrize("grid", [(5, 6, 7), (17, 33, 20)])
@pytest.mark.parametrize("factors", FACTORS)
def test_resample_equals_the_formula(ops, grid, factors):
    g = np.random.default_rng(11)
    x = (1000.0 * g.standard_normal((2,) + grid)).astype(np.float32)
    out = tuple(prep.resample_extent(n, f) for n, f in zip(grid, factors))
    if factors == FACTORS[-1]:
        assert out[0] == 1 and out[2] == 1
    got = ops.prep_resample(dev(x), factors, out).cpu().numpy()
    want = R.ref_resample_linear(x, factors, out)
    assert got.shape == (2,) + out
    # seven fp32 multiply-adds and the rounding of the weights to fp32: 8 2^-24 max |x| per voxel
    bound = 8 * U24 * float(np.abs(x).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"resample {grid} x {factors}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if factors == FACTORS[0]:
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32))
    lab = g.integers(0, 256, size=(1,) + grid).astype(np.uint8)
    lab[0, 0, 0, 0] = 255
    got = ops.prep_resample(dev(lab), factors, out, nearest=True).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, R.ref_resample_nearest(lab, factors, out))


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _brats_set(root):
    """Two subjects, 4 modalities of 40 x 44 x 36 with a zero margin of differing width per side: int16 with scl_slope 0.5,
    t1ce as float32."""
    aff = np.array([[1.0, 0, 0, -20.0], [0, 1.0, 0, -22.0], [0, 0, 1.0, 7.0], [0, 0, 0, 1.0]])
    os.makedirs(os.path.join(root, "src"))
    rows, truth = [], {}
    for k, sn in enumerate(("b1", "b2")):
        margin = ((3 + k, 5), (6, 2 + k), (4, 7 - k))
        vols, seg, body = R.brats_like(30 + k, (40, 44, 36), margin)
        cells, real = [sn], []
        for c, m in enumerate(D.MODALITIES["brats"]):
            cells.append(os.path.join("src", f"{sn}_{m}.nii.gz"))
            if m == "t1ce":
                v = (vols[c].astype(np.float32) * np.float32(0.37))
                R.write_scan(os.path.join(root, cells[-1]), v, affine=aff)
                real.append(v)
            else:
                R.write_scan(os.path.join(root, cells[-1]), vols[c], affine=aff, slope=0.5)
                real.append((vols[c].astype(np.float64) * 0.5).astype(np.float32))
        cells.append(os.path.join("src", f"{sn}_seg.nii.gz"))
        R.write_scan(os.path.join(root, cells[-1]), seg, affine=aff)
        rows.append(cells)
        truth[sn] = (np.stack(real), seg, body)
    return R.write_list(os.path.join(root, "cases.csv"), rows), truth, aff


def _moments_are_0_and_1(arr, mask):
    v = arr.astype(np.float64)[mask]
    assert abs(v.mean()) <= 1e-6 and abs(v.std() - 1.0) <= 1e-6


def test_mission_on_the_device_and_the_round_trip_through_validate_seg(tmp_path):
    root = str(tmp_path)
    lst, truth, aff = _brats_set(root)
    out, split = os.path.join(root, "data"), os.path.join(root, "split")
    entrance.main(["prep", "--task", "brats", "--src_list", lst, "--data_dir", out, "--split_dir", split, "--val_every",
                   "1", "--prep_min_size", "16,16,16"])
    os.makedirs(os.path.join(split, "round2"))
    for name in ("train.txt", "val.txt"):
        open(os.path.join(split, "round2", name), "w").write("b1\nb2\n")
    args = Cf.make_args(dict(Cf.TINY_NET, task="brats", nMod=4, nClass=4, multi_label="brats"), 4, 4, data_dir=out,
                        split_dir=split, round="2", access_type="npy", merge_type="agg", patch_size="16", src_geom=True)
    cube = D.get_data_cube(args)
    assert cube.val_sn == ["b1", "b2"]
    for sn, geo in zip(cube.val_sn, cube.geometry):
        x, seg, body = truth[sn]
        pmin, pmax = tuple(s.start for s in body), tuple(s.stop for s in body)
        assert (geo["pmin"], geo["pmax"], geo["source_shape"]) == (pmin, pmax, (40, 44, 36))
        _, count, total = R.ref_bbox_moments(x, "nonzero")
        mean = [s / n for s, n in zip(total, count)]
        std = [float(np.sqrt(q / n)) for q, n in zip(R.ref_sqdev(x, mean, "nonzero"), count)]
        want = R.ref_standardise_crop(x, pmin, pmax, mean, std, "nonzero")
        for c, m in enumerate(D.MODALITIES["brats"]):
            arr = np.load(os.path.join(out, m, f"{sn}.npy"))
            assert arr.dtype == np.float32 and arr.shape == want[c].shape
            # the device's mean and std are within n 2^-53 relative of these: the fp64 quotient moves by far less than a
            # float32 ulp, so its rounding lands on the same float32 or its neighbour
            assert np.all(np.abs(arr.astype(np.float64) - want[c]) <= np.spacing(np.abs(want[c])))
            assert np.array_equal(arr == 0, want[c] == 0)
            _moments_are_0_and_1(arr, arr != 0)
        assert np.array_equal(np.load(os.path.join(out, "seg", f"{sn}.npy")), seg[body])

    # the round trip the mission exists for: validate_seg puts its maps back onto the source scans
    from efficientq_amd import calibrate as K, synth
    QConv, _, kwQ = Cf.get_conv_class(args)
    model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
    synth.randomise_network(model, 0)
    model.eval()
    K.search_fold_and_remove_bn(model)
    model.to(DEV)
    K.set_fp(model)
    save = os.path.join(root, "val")
    E.validate_seg(model, cube.valloader, "brats", cube.patch_size, 4, fuse="agg", names=cube.val_sn, save_dir=save,
                   multi_label="brats", geometry=cube.geometry)
    for sn, geo in zip(cube.val_sn, cube.geometry):
        g = nifti.read_geometry(os.path.join(save, f"{sn}.nii.gz"))
        assert g["shape"] == (40, 44, 36) and np.allclose(g["affine"], aff)
        vmap, _ = nifti.read_nifti(os.path.join(save, f"{sn}.nii.gz"))
        inside = np.zeros((40, 44, 36), bool)
        inside[tuple(slice(a, b) for a, b in zip(geo["pmin"], geo["pmax"]))] = True
        assert not vmap[~inside].any()


def test_lits_mission_on_the_device_resamples_to_one_spacing(tmp_path):
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "src"))
    g = np.random.default_rng(4)
    aff = np.array([[0.8, 0, 0, -19.0], [0, 0.8, 0, -19.0], [0, 0, 2.5, 40.0], [0, 0, 0, 1.0]])
    zz, yy, xx = np.meshgrid(np.arange(48), np.arange(48), np.arange(30), indexing="ij")
    ct = (-600.0 + 20.0 * zz + 15.0 * yy - 10.0 * xx + 60.0 * g.standard_normal((48, 48, 30))).astype(np.int16)
    seg = ((zz - 24) ** 2 + (yy - 24) ** 2 + (2 * (xx - 15)) ** 2 < 150).astype(np.uint8) * 2
    R.write_scan(os.path.join(root, "src", "l1_ct.nii.gz"), ct, affine=aff)
    R.write_scan(os.path.join(root, "src", "l1_seg.nii.gz"), seg, affine=aff)
    lst = R.write_list(os.path.join(root, "cases.csv"), [["l1", "src/l1_ct.nii.gz", "src/l1_seg.nii.gz"]],
                       head=("subject", "ct", "seg"))
    out, split = os.path.join(root, "data"), os.path.join(root, "split")
    entrance.main(["prep", "--task", "lits", "--src_list", lst, "--data_dir", out, "--split_dir", split, "--val_every", "1",
                   "--prep_spacing", "1.6,1.6,1.6", "--prep_window", "-200,250", "--prep_min_size", "16,16,16"])
    hdr = nifti.read_geometry(os.path.join(root, "src", "l1_ct.nii.gz"))
    factors = tuple(1.6 / s for s in hdr["spacing"])
    grid = tuple(prep.resample_extent(n, f) for n, f in zip((48, 48, 30), factors))
    assert grid == (24, 24, 47)
    x = np.clip(ct.astype(np.float32), np.float32(-200), np.float32(250))[None]
    r = R.ref_resample_linear(x, factors, grid)                         # fp64
    mean, std = r.mean(), r.std()
    want = (r - mean) / std
    arr = np.load(os.path.join(out, "ct", "l1.npy"))
    assert arr.shape == grid and arr.dtype == np.float32               # mask `all`: the box is the grid, no restore entry
    assert not os.path.exists(os.path.join(out, D.RESTORE_FILE))
    # e = the resampling bound; mean and std of the device's volume move by at most e each, then one float32 rounding
    e = 8 * U24 * 250.0
    tol = (2.0 + np.abs(want[0])) * e / std + np.spacing(np.abs(want[0]).astype(np.float32))
    err = np.abs(arr.astype(np.float64) - want[0])
    print(f"lits: max err {err.max():.3e}, least tolerance {tol.min():.3e}")
    assert np.all(err <= tol)
    _moments_are_0_and_1(arr, np.ones(grid, bool))
    assert np.array_equal(np.load(os.path.join(out, "seg", "l1.npy")), R.ref_resample_nearest(seg[None], factors, grid)[0])
    geo = nifti.read_geometry(os.path.join(out, "grid", "l1.nii.gz"))
    assert geo["shape"] == grid and np.allclose(geo["spacing"], (1.6, 1.6, 1.6), rtol=1e-6, atol=0)
    assert np.allclose(geo["affine"], prep.resample_affine(hdr["affine"], factors), rtol=1e-6, atol=1e-5)
    assert nifti.read_nifti(os.path.join(out, "grid", "l1.nii.gz"))[0].all()
    args = Cf.make_args(Cf.TINY_NET, 4, 4, data_dir=out, split_dir=split, access_type="npy", merge_type=None,
                        patch_size="16", src_geom=True)
    cube = D.get_data_cube(args)
    assert cube.val_sn == ["l1"] and cube.geometry[0]["source_shape"] == grid and "pmin" not in cube.geometry[0]
    assert cube.geometry[0]["spacing"] == pytest.approx((1.6, 1.6, 1.6), rel=1e-6)
