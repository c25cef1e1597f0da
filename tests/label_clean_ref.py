"""TEST-ONLY numpy restatement of the --post rules (effq_label_clean) and of the tallies of a label map
(effq_label_tallies): the yardstick of test_label_clean_gpu, test_post_cpu and test_post_gpu.  Everything is integer, so
every comparison against it is bit for bit.

A rule is (labels, op, n, to) - config.PostRule.  Its mask is "the voxel's value is one of labels"; the components of the
mask are named by their first voxel (least linear index d*H*W + h*W + w); `largest` keeps the component of the largest
size, of equal sizes the one named least, and gives every other voxel of the mask the value `to`; `min` gives `to` to the
voxels of every component of fewer than n voxels.  Rules apply in order, each to the map the previous one left."""
import numpy as np

try:
    from scipy import ndimage
except ImportError:          # the cross-check against scipy is then not made
    ndimage = None


def _offsets(connectivity):
    assert connectivity in (6, 26)
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)
            if (a, b, c) != (0, 0, 0) and (connectivity == 26 or abs(a) + abs(b) + abs(c) == 1)]


def first_voxels(mask, connectivity=26):
    """int64 array of the mask's shape: -1 outside the mask, else the least linear index of the voxel's component.  Min
    propagation over the neighbourhood; between two sweeps every voxel also takes the name of the voxel its name points
    at (a voxel of its own component), which only shortens long paths."""
    m = np.asarray(mask).astype(bool)
    assert m.ndim == 3
    D, H, W = m.shape
    big = np.int64(m.size)
    name = np.where(m, np.arange(m.size, dtype=np.int64).reshape(m.shape), big)
    fg = np.flatnonzero(m.reshape(-1))
    offs = _offsets(connectivity)
    while True:
        pad = np.pad(name, 1, constant_values=big)
        new = name.copy()
        for a, b, c in offs:
            np.minimum(new, pad[1 + a:1 + a + D, 1 + b:1 + b + H, 1 + c:1 + c + W], out=new)
        new[~m] = big
        flat = new.reshape(-1)
        for _ in range(4):
            flat[fg] = flat[flat[fg]]
        if np.array_equal(new, name):
            break
        name = new
    out = np.where(m, name, -1)
    if ndimage is not None:      # numbered in the order of their first voxels the components are scipy's
        want, n = ndimage.label(m, np.ones((3, 3, 3)) if connectivity == 26 else None)
        ids = np.unique(out[m])
        assert n == len(ids)
        assert np.array_equal(np.where(m, np.searchsorted(ids, out) + 1, 0), want)
    return out


def component_sizes(names):
    """(first voxels ascending, sizes) of the components of a first_voxels array."""
    ids, sizes = np.unique(names[names >= 0], return_counts=True)
    return ids, sizes


def clean_rule(label_map, rule, connectivity=26):
    """(map after the rule, (components of the mask, voxels relabelled))."""
    labels, op, n, to = rule
    a = np.asarray(label_map)
    assert a.dtype == np.uint8 and a.ndim == 3 and 0 <= to <= 255 and to not in labels and min(labels) >= 1
    names = first_voxels(np.isin(a, list(labels)), connectivity)
    ids, sizes = component_sizes(names)
    if len(ids) == 0:
        return a.copy(), (0, 0)
    if op == "largest":
        keep = ids[np.argmax(sizes)]             # the first of the largest: ids ascend, so the least first voxel
        lose = (names >= 0) & (names != keep)
    else:
        assert op == "min" and n >= 1
        small = ids[sizes < n]
        lose = np.isin(names, small)
    out = a.copy()
    out[lose] = to
    return out, (len(ids), int(lose.sum()))


def clean(label_map, rules, connectivity=26):
    """(cleaned map uint8, stats int64 R x 2) of the rules applied in order."""
    a = np.ascontiguousarray(label_map)
    stats = []
    for rule in rules:
        a, st = clean_rule(a, rule, connectivity)
        stats.append(st)
    return a, np.asarray(stats, dtype=np.int64).reshape(len(rules), 2)


def tallies(pred, truth, lut, C):
    """C x 4 int64 TP, FP, FN, TN: the class bits of pred are lut[pred]; the truth is a map read through lut, or C
    planes (C x pred's shape), non-zero = the class holds the voxel."""
    lut = np.asarray(lut, dtype=np.int64)
    assert lut.shape == (256,)
    p = lut[np.asarray(pred)]
    truth = np.asarray(truth)
    out = np.zeros((C, 4), dtype=np.int64)
    for c in range(C):
        pc = (p >> c) & 1 != 0
        tc = ((lut[truth] >> c) & 1 != 0) if truth.shape == p.shape else truth[c] != 0
        out[c] = [(pc & tc).sum(), (pc & ~tc).sum(), (~pc & tc).sum(), (~pc & ~tc).sum()]
    return out


def class_lut(rule, C):
    """The table of the validation: argmax - class c is the value c; brats - WT = {1, 2, 4}, TC = {1, 4}, ET = {4}."""
    lut = [0] * 256
    if rule == "argmax":
        for c in range(C):
            lut[c] = 1 << c
    else:
        assert rule == "brats" and C == 3
        lut[1], lut[2], lut[4] = 0b011, 0b001, 0b111
    return lut
