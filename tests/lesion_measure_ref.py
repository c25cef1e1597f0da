"""The yardstick of effq_label_lesion_measures and of the host side of --lesion_measures, in numpy and
scipy.ndimage.label: the components of every class plane with their first voxel, size, overlap, coordinate sums and box;
the greatest fp32 E over all pairs of voxels of a component, term by term as the kernel rounds it (farthest_brute), and
over the ends of its lines only (farthest_lines); the rule that picks one pair among those of the greatest E; and the
formulas of lesions.csv and lesion_detect.csv, written down independently of efficientq_amd.lesion_measures."""
import math

import numpy as np
from scipy import ndimage

F32 = np.float32
WORDS = 13
SPACINGS = ((1.0, 1.0, 1.0), (0.7, 0.7, 2.5), (0.9765625, 0.9765625, 5.0))
BINS = (("<5", 0.0, 5.0), ("5-10", 5.0, 10.0), ("10-20", 10.0, 20.0), (">=20", 20.0, math.inf))
COLUMNS = ("subject", "class", "labels", "kind", "lesion", "d", "h", "w", "size", "overlap", "vol_ml", "cd", "ch", "cw",
           "x_mm", "y_mm", "z_mm", "box_lo", "box_hi", "diam_mm", "diam_from", "diam_to", "plane", "plane_diam_mm",
           "plane_from", "plane_to")


def weights(spacing):
    """The fp32 axis weights float32(float64(spacing) ** 2)."""
    return tuple(F32(np.float64(s) ** 2) for s in spacing)


def components(mask, conn):
    """(labels, n) of scipy.ndimage.label at 6- or 26-connectivity: component k + 1 is the one whose first voxel has the
    k-th smallest linear index."""
    return ndimage.label(mask, ndimage.generate_binary_structure(3, 3 if conn == 26 else 1))


def class_planes(pred, truth, classes):
    """The P masks of a call: the predicted mask of every class, then (truth not None) the label mask of every class."""
    maps = (pred,) if truth is None else (pred, truth)
    return [np.isin(m, labels) for m in maps for labels in classes]


def energy(a, b, w):
    """E (n x m, fp32) between the voxels a (n x 3) and b (m x 3): every product and sum rounded to fp32."""
    d = a[:, None, :].astype(np.int64) - b[None, :, :].astype(np.int64)
    sq = (d * d).astype(F32)                    # exact: every square is below 2^24
    w = [F32(v) for v in w]
    return (w[0] * sq[..., 0] + w[1] * sq[..., 1]) + w[2] * sq[..., 2]


def farthest(vox, w, axis, chunk=256):
    """Over all pairs of the voxels `vox` (n x 3 coordinates, in ascending linear order), and over the pairs that share
    coordinate `axis`: (E, a, b) with E the greatest fp32 E, a the least position that any pair of that E holds and b
    the least partner of a at that E (positions into vox, a <= b).  Returns the two triples."""
    vox = np.asarray(vox, dtype=np.int64)
    best = [None, None]
    for i in range(0, len(vox), chunk):
        e = energy(vox[i:i + chunk], vox, w)
        same = vox[i:i + chunk, None, axis] == vox[None, :, axis]
        for kind, ok in ((0, None), (1, same)):
            ek = e if ok is None else np.where(ok, e, F32(-1))
            top = ek.max()
            if best[kind] is not None and top < best[kind][0]:
                continue
            r, c = np.nonzero(ek == top)
            lo, hi = np.minimum(r + i, c), np.maximum(r + i, c)
            a = int(lo.min())
            b = int(hi[lo == a].min())
            if best[kind] is None or top > best[kind][0] or (a, b) < best[kind][1:]:
                best[kind] = (F32(top), a, b)
    return best


def line_ends(comp, axis):
    """The voxels of the component mask `comp` that end one of its lines along w (along h when the slices are stacked
    along w, axis 2): their neighbour before or after along the line is not in the component."""
    line = 1 if axis == 2 else 2
    pad = np.pad(comp, [(1, 1) if a == line else (0, 0) for a in range(3)])
    n = comp.shape[line]
    before, after = np.take(pad, range(0, n), axis=line), np.take(pad, range(2, n + 2), axis=line)
    return comp & ~(before & after)


def farthest_brute(comp, w, axis):
    """farthest over every voxel of the component mask; positions turned into linear indices of the volume."""
    return _linear(comp, np.argwhere(comp), w, axis)


def farthest_lines(comp, w, axis):
    """farthest over the line ends of the component mask only."""
    return _linear(comp, np.argwhere(line_ends(comp, axis)), w, axis)


def _linear(comp, vox, w, axis):
    lin = np.ravel_multi_index(vox.T, comp.shape)
    return [(e, int(lin[a]), int(lin[b])) for e, a, b in farthest(vox, w, axis)]


def measures(pred, truth, classes, conn, spacing, axis, far=farthest_lines):
    """What the call returns for the maps, per plane: (nrows (P), [rows n x 3 int32], [meas n x 13 int64], [bits n x 2
    uint32: the fp32 bits of the greatest E in 3-D and inside a slice])."""
    planes = class_planes(pred, truth, classes)
    C, w = len(classes), weights(spacing)
    nrows, rows, meas, bits = [], [], [], []
    for q, mask in enumerate(planes):
        other = None if truth is None else planes[q + C if q < C else q - C]
        lab, n = components(mask, conn)
        boxes = ndimage.find_objects(lab)
        r, m, eb = np.zeros((n, 3), np.int32), np.zeros((n, WORDS), np.int64), np.zeros((n, 2), np.uint32)
        for k in range(n):
            box = boxes[k]
            lo = np.array([s.start for s in box])
            comp = lab[box] == k + 1
            vox = np.argwhere(comp) + lo
            r[k] = (np.ravel_multi_index(vox[0], mask.shape), len(vox), 0 if other is None else int(other[box][comp].sum()))
            m[k, 0:3], m[k, 3:6], m[k, 6:9] = vox.sum(0), vox.min(0), vox.max(0)
            for kind, (e, a, b) in enumerate(far(comp, w, axis)):
                pa, pb = (np.array(np.unravel_index(v, comp.shape)) + lo for v in (a, b))
                m[k, 9 + 2 * kind] = np.ravel_multi_index(pa, mask.shape)
                m[k, 10 + 2 * kind] = np.ravel_multi_index(pb, mask.shape)
                eb[k, kind] = np.array(e, F32).view(np.uint32)
        nrows.append(n)
        rows.append(r)
        meas.append(m)
        bits.append(eb)
    return np.array(nrows, np.int64), rows, meas, bits


def pair_bits(a, b, shape, w):
    """The fp32 bits of E between the voxels of linear indices a and b."""
    pa, pb = (np.array(np.unravel_index(int(v), shape))[None] for v in (a, b))
    return int(energy(pa, pb, w).view(np.uint32)[0, 0])


# ---- the host formulas ---------------------------------------------------------------------------------------------------
def g7(v):
    return "%.7g" % v


def triple(v):
    return " ".join(str(int(x)) for x in v)


def expected_lesions(subject, classes, with_truth, rows, meas, shape, spacing, affine, axis):
    """(cells, diameters): the cells of lesions.csv of one subject as the file holds them (strings), all columns, and
    the fp64 3-D diameter behind every row (the printed cell has seven digits only)."""
    C = len(classes)
    A = np.asarray(affine, np.float64)
    out, diams = [], []
    for c, labels in enumerate(classes):
        for kind, q in ((("label", C + c), ("pred", c)) if with_truth else (("pred", c),)):
            for k, (r, m) in enumerate(zip(rows[q], meas[q])):
                first = np.unravel_index(int(r[0]), shape)
                cen = [int(m[a]) / int(r[1]) for a in range(3)]
                xyz = [sum(A[i, a] * cen[a] for a in range(3)) + A[i, 3] for i in range(3)]
                ends = [np.unravel_index(int(m[j]), shape) for j in (9, 10, 11, 12)]
                diam = [math.sqrt(sum((spacing[a] * (int(q1[a]) - int(p1[a]))) ** 2 for a in range(3)))
                        for p1, q1 in ((ends[0], ends[1]), (ends[2], ends[3]))]
                out.append([subject, str(c), triple(labels), kind, str(k + 1)] + [str(int(v)) for v in first] +
                           [str(int(r[1])), str(int(r[2])), g7(int(r[1]) * spacing[0] * spacing[1] * spacing[2] / 1000.0)] +
                           [g7(v) for v in cen] + [g7(v) for v in xyz] + [triple(m[3:6]), triple(m[6:9]), g7(diam[0]),
                                                                         triple(ends[0]), triple(ends[1]), "dhw"[axis],
                                                                         g7(diam[1]), triple(ends[2]), triple(ends[3])])
                diams.append(diam[0])
    return out, diams


def expected_detect(classes, lesions, diams):
    """The cells of lesion_detect.csv from the cells and diameters of expected_lesions (all subjects)."""
    col = {k: i for i, k in enumerate(COLUMNS)}
    out = []
    for c, labels in enumerate(classes):
        for name, lo, hi in BINS:
            mine = [r for r, d in zip(lesions, diams) if r[col["class"]] == str(c) and lo <= d < hi]
            label = [r for r in mine if r[col["kind"]] == "label"]
            out.append([str(c), triple(labels), name, str(len(label)),
                        str(sum(1 for r in label if int(r[col["overlap"]]) > 0)),
                        str(sum(1 for r in mine if r[col["kind"]] == "pred" and int(r[col["overlap"]]) == 0))])
    return out

