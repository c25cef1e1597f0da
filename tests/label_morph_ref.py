"""TEST-ONLY numpy / scipy restatement of a chain of --post rules with the morphological ops (effq_label_post): the
yardstick of test_post_morph_cpu and test_post_morph_gpu.  Everything is integer or boolean, so every comparison against
it is bit for bit.  `largest` and `min` are label_clean_ref's.

A rule is (labels, op, n, to) - config.PostRule - and its mask M is "the voxel's value is one of labels".  With
B_R = {(dd, dh, dw): dd^2 + dh^2 + dw^2 <= R^2}:

  fill    every hole of M becomes `to`: scipy.ndimage.binary_fill_holes with the structure of the dual connectivity (the
          faces-only cross when the rules use 26, the full cube when they use 6).  stats = (holes, voxels)
  close   the voxels of (M + B_R) - B_R outside M become `to`: dilation, then erosion, of M padded by R voxels of
          background on every side (the infinite grid, everything outside the volume background), cropped
  open    the voxels of M outside (M - B_R) + B_R become `to`: scipy's binary_opening with border_value 0
          stats of both = (voxels of M before the rule, voxels relabelled)
          Beyond SCIPY_MAX_RADIUS scipy's structuring element is out of reach (the ball of radius 32 has 137 065 offsets
          per voxel); there the same sets come from thresholds of the exact squared distance (edt_sq below),
          which test_post_morph_cpu holds to the scipy forms at the radii both can do.

Rules apply in order, each to the map the previous one left."""
import numpy as np
from scipy import ndimage

from tests import label_clean_ref as R


def ball(radius):
    r = int(radius)
    g = np.arange(-r, r + 1)
    return (g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) <= r * r


def holes(mask, connectivity=26):
    """The voxels of the holes of `mask` (bool), and how many holes they make: the components of the complement, at the
    dual connectivity, without a voxel on a face of the volume."""
    m = np.asarray(mask).astype(bool)
    dual = ndimage.generate_binary_structure(3, 1 if connectivity == 26 else 3)
    filled = ndimage.binary_fill_holes(m, dual)
    inside = filled & ~m
    return inside, int(ndimage.label(inside, dual)[1])


SCIPY_MAX_RADIUS = 5     # beyond it scipy's structuring element of (2 R + 1)^3 offsets per voxel is out of reach


def edt_sq(sites):
    """Exact squared Euclidean distance (int64) of every voxel to the nearest True voxel of `sites`; a value larger than
    any squared distance of the array throughout when there is none.  scipy's transform is exact in the voxel it finds
    and returns the fp64 square root of an integer below 2^31: its square is off by a few ulp, far from one half."""
    s = np.asarray(sites).astype(bool)
    big = np.int64(4 * sum(n * n for n in s.shape) + 1)
    if not s.any():
        return np.full(s.shape, big)
    return np.rint(ndimage.distance_transform_edt(~s) ** 2).astype(np.int64)


def close_by_distance(mask, radius):
    """The issue's formulas: dilate(X) = {edt_sq(., X) <= R^2}, erode(X) = {edt_sq(., not X) > R^2}, on the padded plane."""
    m = np.asarray(mask).astype(bool)
    r = int(radius)
    grown = edt_sq(np.pad(m, r)) <= r * r
    back = edt_sq(~grown) > r * r
    return back[r:r + m.shape[0], r:r + m.shape[1], r:r + m.shape[2]]


def open_by_distance(mask, radius):
    m = np.asarray(mask).astype(bool)
    r = int(radius)
    shrunk = edt_sq(~np.pad(m, r)) > r * r
    back = edt_sq(shrunk) <= r * r
    return back[r:r + m.shape[0], r:r + m.shape[1], r:r + m.shape[2]]


def close(mask, radius):
    m = np.asarray(mask).astype(bool)
    r = int(radius)
    if r > SCIPY_MAX_RADIUS:
        return close_by_distance(m, r)
    b = ball(r)
    grown = ndimage.binary_dilation(np.pad(m, r), b)
    back = ndimage.binary_erosion(grown, b)          # border_value 0: the pad keeps it from reaching the volume
    return back[r:r + m.shape[0], r:r + m.shape[1], r:r + m.shape[2]]


def open_(mask, radius):
    m = np.asarray(mask).astype(bool)
    if int(radius) > SCIPY_MAX_RADIUS:
        return open_by_distance(m, radius)
    return ndimage.binary_opening(m, ball(radius))   # border_value 0


def morph_rule(label_map, rule, connectivity=26):
    """(map after the rule, (stats 0, stats 1))."""
    labels, op, n, to = rule
    a = np.asarray(label_map)
    assert a.dtype == np.uint8 and a.ndim == 3 and min(labels) >= 1
    m = np.isin(a, list(labels))
    if op == "fill":
        assert to in labels
        change, first = holes(m, connectivity)
    elif op == "close":
        assert to in labels and 1 <= n <= 32
        change, first = close(m, n) & ~m, int(m.sum())
    else:
        assert op == "open" and to not in labels and 0 <= to <= 255 and 1 <= n <= 32
        change, first = m & ~open_(m, n), int(m.sum())
    out = a.copy()
    out[change] = to
    return out, (first, int(change.sum()))


def post(label_map, rules, connectivity=26):
    """(map uint8, stats int64 R x 2) of the rules applied in order."""
    a = np.ascontiguousarray(label_map)
    stats = []
    for rule in rules:
        a, st = (R.clean_rule if rule[1] in ("largest", "min") else morph_rule)(a, rule, connectivity)
        stats.append(st)
    return a, np.asarray(stats, dtype=np.int64).reshape(len(rules), 2)
