"""The numpy restatement of effq_prep_bins and effq_prep_joint_hist (csrc/prep_register.hip), and a stand-in `ops`."""
import numpy as np
import torch

from tests import prep_align_ref as A
from tests import prep_window_ref as Q

BINS, SKIP = 32, 255


def bins(x, lo, scale, mask_nonzero=False):
    """t = (x - lo) * scale in fp32; NaN -> SKIP, t < 0 -> 0, t >= BINS -> BINS - 1, else int(t); 0 under the mask -> SKIP."""
    with np.errstate(all="ignore"):
        t = (np.asarray(x, np.float32) - np.float32(lo)) * np.float32(scale)
        b = np.clip(np.where(np.isnan(t), 0, t), 0, BINS - 1).astype(np.uint8)      # the cast truncates, as (int)t does
    return np.where(np.isnan(t) | (np.asarray(x) == 0 if mask_nonzero else False), np.uint8(SKIP), b)


def joint_hist(fbin, mov, matrices, lo, scale, stride=(1, 1, 1)):
    """(hist [K, BINS, BINS], inside [K]: sampled voxels with a bin inside mov's field of view, lost [K]: NaN samples)."""
    ms = np.asarray(matrices, np.float64).reshape(-1, 3, 4)
    cut = tuple(slice(None, None, s) for s in stride)
    bf = fbin[cut]
    hist, inside, lost = np.zeros((len(ms), BINS, BINS), np.int64), [], []
    for k, m in enumerate(ms):
        fov = A.field_of_view(A.coordinates(m, fbin.shape), mov.shape)[cut] & (bf < BINS)
        bm = bins(A.align(mov, m, fbin.shape)[0][cut], lo, scale)
        ok = fov & (bm != SKIP)
        np.add.at(hist[k], (bf[ok], bm[ok]), 1)
        inside.append(int(fov.sum()))
        lost.append(int((fov & ~ok).sum()))
    return hist, inside, lost


class RegisterMixin:
    def prep_bins(self, x, lo, scale, mask_nonzero=False):
        return torch.from_numpy(bins(x.numpy(), lo, scale, mask_nonzero))

    def prep_joint_hist(self, fbin, mov, matrices, lo, scale, stride=(1, 1, 1)):
        return torch.from_numpy(joint_hist(fbin.numpy(), mov.numpy(), matrices, lo, scale, stride)[0])

    def prep_quantiles(self, x, qs, mask="nonzero"):
        got = [Q.ref_stats(a, qs, mask) for a in x.numpy()]
        return torch.tensor([n for n, _ in got]), torch.from_numpy(np.stack([s for _, s in got]))


PAIR_SHAPE = (24, 28, 32)
PAIR_THETA = (1.8, -1.5, 1.9, float(np.deg2rad(3.0)), 0.0, float(np.deg2rad(-2.6)))      # 3.0 mm and 4.0 degrees


def blobs(shape=PAIR_SHAPE, seed=7, count=12):
    g = np.random.default_rng(seed)
    grid = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij"), -1)
    v = np.full(shape, 100.0)
    for _ in range(count):
        c, s = g.uniform(0.15, 0.85, 3) * shape, g.uniform(2.5, 6.0) * min(shape) / 24.0
        v += g.uniform(200.0, 600.0) * np.exp(-((grid - c) ** 2).sum(-1) / (2.0 * s * s))
    return v


def synthetic_pair(true_matrix, shape=PAIR_SHAPE, seed=7):
    """(fixed, moving): `moving` is a decreasing non-linear function of `fixed` seen through `true_matrix`."""
    fixed = blobs(shape, seed).astype(np.float32)
    g = (2000.0 / (1.0 + (fixed.astype(np.float64) / 300.0) ** 2)).astype(np.float32)
    inv = np.linalg.inv(np.vstack([true_matrix, [0.0, 0.0, 0.0, 1.0]]))[:3]
    return fixed, A.align(g, inv, shape)[0]
