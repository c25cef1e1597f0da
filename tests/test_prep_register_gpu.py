"""effq_prep_bins and effq_prep_joint_hist against the numpy restatement, the search on both backends, the mission."""
import numpy as np
import pytest
import torch

from efficientq_amd import entrance, ops_align, ops_register, prep
from efficientq_amd.hip_ops import get_ops
from tests import prep_align_ref as A
from tests import prep_register_ref as R
from tests import test_prep_register_cpu as C
from tests.test_prep_cpu import write_list

pytestmark = pytest.mark.gpu
LO, SCALE = -512.0, 2.0 ** -5           # bins of width 32 from -512 to 512: the edges are exact in fp32
# greatest corner displacement between M(theta) and the truth, reference voxels, measured on the numpy stand-in
RECOVERY_MEASURED = 0.0996236180415503


@pytest.fixture(scope="module")
def ops():
    return get_ops("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def candidates(base, K):
    """K distinct matrices around `base`; the last of more than one puts every voxel outside the field of view."""
    ms = np.stack([base] * K)
    ms[:, :, 3] += 0.37 * np.arange(K)[:, None] * np.array([1.0, -0.5, 0.25])
    ms[:, 0, 1] += 0.01 * np.arange(K)
    ms[-1, :, 3] += 1000.0 * (K > 1)
    return ms


def volumes(n_ref, n_mov, constant=False, seed=0):
    """(fbin with a row and the tail W % 4 not sampled, mov with values past lo and hi, bin edges, NaN and Inf)."""
    g = np.random.default_rng(seed)
    b = g.integers(0, R.BINS, n_ref).astype(np.uint8)
    b[g.random(n_ref) < 0.1] = R.SKIP
    b[n_ref[0] // 2, n_ref[1] // 3, :] = R.SKIP
    b[:, :, n_ref[2] - n_ref[2] % 4:] = R.SKIP
    x = g.uniform(-700.0, 700.0, n_mov).astype(np.float32)
    edge = g.random(n_mov) < 0.2
    x[edge] = (LO + 32.0 * g.integers(0, 33, n_mov))[edge]
    x.reshape(-1)[[5, x.size // 2, x.size - 3]] = np.nan, np.inf, -np.inf
    return b, np.full(n_mov, 100.0, np.float32) if constant else x


M_OBL, N_SRC, N_REF = C.H.oblique()
BIG = prep.align_matrix("s", "m", A.affine((1.6, 1.8, 1.9), (2.0, -3.0, 1.5), A.rotation(1, 4.0)), A.affine((1.0, 1.0, 1.0)))
CASES = {       # name -> (reference shape, moving shape, matrices, stride, constant moving volume)
    "oblique, K = 13": (N_REF, N_SRC, candidates(M_OBL, 13), (1, 1, 1), False),
    "oblique, K = 16, stride 2 3 1": (N_REF, N_SRC, candidates(M_OBL, 16), (2, 3, 1), False),
    "oblique, K = 1, stride 4 4 4": (N_REF, N_SRC, candidates(M_OBL, 1), (4, 4, 4), False),
    "identity on equal grids": ((9, 10, 14), (9, 10, 14), np.eye(4)[None, :3], (1, 1, 1), False),
    # 72 x 128 x 32 items of four: beyond the 1024 x 256 items of one trip of the capped grid
    "second trip": ((72, 128, 128), (40, 70, 70), candidates(BIG, 2), (1, 1, 1), False),
    "constant moving volume, K = 13": (N_REF, N_SRC, candidates(M_OBL, 13), (1, 1, 1), True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_joint_histogram_equals_the_restatement_exactly(ops, name):
    n_ref, n_mov, ms, stride, constant = CASES[name]
    fbin, mov = volumes(n_ref, n_mov, constant)
    want, inside, lost = R.joint_hist(fbin, mov, ms, LO, SCALE, stride)
    hist = ops_register.prep_joint_hist(ops, dev(fbin), dev(mov), ms, LO, SCALE, stride)
    got = hist.cpu().numpy()
    assert got.shape == (len(ms), R.BINS, R.BINS) and got.dtype == np.int64 and np.array_equal(got, want)
    assert got.sum((1, 2)).tolist() == [n - k for n, k in zip(inside, lost)] and inside[0] > 0 and inside[1:][-1:] in ([], [0])
    assert not constant or (got.sum(1) > 0).sum(1).max() == 1          # every sample of a candidate in one column
    assert torch.equal(ops_register.prep_joint_hist(ops, dev(fbin), dev(mov), ms, LO, SCALE, stride), hist)


@pytest.mark.parametrize("mask_nonzero", [False, True])
def test_bins_equal_the_restatement_exactly(ops, mask_nonzero):
    x = volumes((1, 1, 1), (7, 9, 13), seed=3)[1]                  # W = 13: a tail of one
    x.reshape(-1)[::7] = 0.0
    x[1, 2, 3] = -0.0
    got = ops_register.prep_bins(ops, dev(x), LO, SCALE, mask_nonzero).cpu().numpy()
    want = R.bins(x, LO, SCALE, mask_nonzero)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert (want == R.SKIP).sum() == (1 + (x == 0).sum() if mask_nonzero else 1) and {0, R.BINS - 1} <= set(want.reshape(-1))


def test_the_same_search_on_both_backends(ops):
    (on_device, err, _), (on_host, _, _) = C.registered_pair(ops, dev), C.registered_pair(C.RegisterOps())
    assert on_device[:1] + on_device[2:5] == on_host[:1] + on_host[2:5]          # theta; both NMI and the launches
    assert np.array_equal(on_device.matrix, on_host.matrix) and on_device.converged
    assert err <= 2 * RECOVERY_MEASURED < 1.0 and on_device.nmi_after > on_device.nmi_before


def test_the_coarse_level_smooths_both_volumes_and_hands_theta_on(ops):
    """32^3 keeps the stride-2 level.  The bar is twice the 0.1366 voxels measured on the stand-in with numpy's filter."""
    got, err, levels = C.registered_pair(ops, dev, (32, 32, 32))
    assert levels == [2, 1] and err <= 2 * 0.136584476518502 < 1.0 and got.nmi_after > got.nmi_before and got.converged


def test_prep_mission_on_the_device(ops, tmp_path, capsys):
    rows, truth = C.register_subjects(str(tmp_path))
    entrance.main(["prep", "--task", "brats", "--src_list", write_list(tmp_path / "cases.csv", rows), "--data_dir",
                   str(tmp_path / "out"), "--prep_min_size", "8,8,8", "--prep_align", "t1ce", "--prep_register", "rigid"])

    def plane(raw, matrix, lo, hi, mean, std):
        x, _ = ops_align.prep_align(ops, dev(raw), matrix, R.PAIR_SHAPE)
        return ops.prep_standardise_crop(x[None], lo, hi, mean, std, "nonzero")[0].cpu().numpy()
    C.check_mission(str(tmp_path / "out"), truth, plane, capsys.readouterr().out)
