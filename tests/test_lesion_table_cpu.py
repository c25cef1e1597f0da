"""Per-lesion validation table (--lesion_table), host side (no GPU): the flag and its YAML key, the C-ABI rows of the
table kernels, lesions.csv and the size summary, and the yardstick the GPU tests compare against - ref_table, one record
per component built on the numpy labeller of test_seg_lesions_cpu - on hand-made cases with known answers and, where
scipy imports, against scipy.ndimage.label + numpy.bincount."""
import csv
import os
import re

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, evaluate as E
from tests.test_seg_lesions_cpu import ref_label

try:
    from scipy import ndimage
except ImportError:          # the extra assertions against scipy are then not made
    ndimage = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the yardstick ------------------------------------------------------------------------------------------------
def ref_rows(mask, other=None, connectivity=26):
    """n x 3 int64, one row per component of `mask` in ascending order of its first voxel: first voxel (linear index),
    size, and the voxels of the component that `other` holds too (0 without `other`)."""
    m = np.asarray(mask) != 0
    lab = ref_label(m, connectivity).reshape(-1).astype(np.int64)
    firsts = np.unique(lab[lab > 0]) - 1                       # a label is 1 + the component's least index
    size = np.bincount(lab, minlength=m.size + 1)[firsts + 1]
    hit = lab[np.asarray(other).reshape(-1) != 0] if other is not None else np.zeros(0, np.int64)
    overlap = np.bincount(hit, minlength=m.size + 1)[firsts + 1]
    rows = np.stack([firsts, size, overlap], axis=1).astype(np.int64).reshape(-1, 3)
    if ndimage is not None:      # scipy numbers the components in raster order of their first voxel
        want, n = ndimage.label(m, np.ones((3, 3, 3)) if connectivity == 26 else None)
        assert n == len(rows)
        assert np.array_equal(np.bincount(want.reshape(-1), minlength=n + 1)[1:], rows[:, 1])
        assert np.array_equal(want.reshape(-1)[rows[:, 0]], np.arange(1, n + 1))
        if other is not None:
            both = want.reshape(-1)[np.asarray(other).reshape(-1) != 0]
            assert np.array_equal(np.bincount(both, minlength=n + 1)[1:], rows[:, 2])
    return rows


def ref_table(pred, gt, connectivity=26):
    """(rows of the predicted mask, rows of the label mask) of one class: ref_rows of each against the other."""
    return ref_rows(pred, gt, connectivity), ref_rows(gt, pred, connectivity)


def lin(shape, d, h, w):
    return (d * shape[1] + h) * shape[2] + w


# ---- the flag and the symbols -------------------------------------------------------------------------------------
def test_parser_knows_lesion_table_and_a_yaml_key_sets_it(tmp_path):
    assert Cf.build_parser().parse_args(["ptq"]).lesion_table is False
    assert Cf.build_parser().parse_args(["ptq", "--lesion_table"]).lesion_table is True
    assert Cf.make_args(Cf.TINY_NET, 4, 4).lesion_table is False
    cfg = tmp_path / "table.yaml"
    cfg.write_text("lesion_table: true\ntask: lits\n")
    args = Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["ptq"]))
    assert args.lesion_table is True and args.task == "lits" and args.is_cc is False


def _ctype(decl):
    decl = decl.strip()
    if "*" in decl:
        return _lib._P
    return {"int": _lib._I, "float": _lib._F, "size_t": _lib._SZ}[decl.split()[0]]


def test_table_symbols_in_header_and_lib_have_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, res in (("effq_cc_table_ws_bytes", "size_t"), ("effq_cc_table", "int"), ("effq_seg_lesion_table", "int")):
        m = re.search(rf"\b{res} {name}\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        want = [_ctype(a) for a in m.group(1).split(",")]
        got_res, got = _lib.SIGNATURES[name]
        assert got == want, name
        assert got_res == (_lib._SZ if res == "size_t" else _lib._I)
    assert len(_lib.SIGNATURES["effq_cc_table"][1]) == 12 and len(_lib.SIGNATURES["effq_seg_lesion_table"][1]) == 17
    chunk = re.search(r"#define EFFQ_CC_TABLE_CHUNK (\d+)", hdr)
    assert chunk and int(chunk.group(1)) == _lib.CC_TABLE_CHUNK
    assert _lib.LESION_TABLE_ROWS > 0


# ---- ref_table on hand-made cases ---------------------------------------------------------------------------------
def test_blobs_touching_at_a_corner_are_one_row_at_26_and_two_at_6():
    shape = (6, 7, 8)
    m = np.zeros(shape, np.uint8)
    m[1:3, 1:3, 1:3] = 1
    m[3:5, 3:5, 3:5] = 1                      # (2, 2, 2) and (3, 3, 3) share a corner only
    assert ref_rows(m, None, 26).tolist() == [[lin(shape, 1, 1, 1), 16, 0]]
    assert ref_rows(m, None, 6).tolist() == [[lin(shape, 1, 1, 1), 8, 0], [lin(shape, 3, 3, 3), 8, 0]]
    assert ref_rows(m, m, 6)[:, 2].tolist() == [8, 8]


def test_a_predicted_blob_over_two_label_blobs():
    shape = (5, 6, 12)
    gt = np.zeros(shape, np.uint8)
    gt[1:3, 1:3, 1:3] = 1
    gt[1:3, 1:3, 8:10] = 1
    pred = np.zeros_like(gt)
    pred[2, 2, 2:9] = 1                       # one bar through both: (2, 2, 2) of the first, (2, 2, 8) of the second
    pr, gr = ref_table(pred, gt)
    assert pr.tolist() == [[lin(shape, 2, 2, 2), 7, 2]]
    assert gr.tolist() == [[lin(shape, 1, 1, 1), 8, 1], [lin(shape, 1, 1, 8), 8, 1]]
    pred[4, 5, 11] = 1                        # a false lesion
    pr, gr = ref_table(pred, gt)
    assert pr.tolist() == [[lin(shape, 2, 2, 2), 7, 2], [lin(shape, 4, 5, 11), 1, 0]]
    pred[2, 2, 2:9] = 0                       # the bar gone: both labelled lesions missed
    pr, gr = ref_table(pred, gt)
    assert pr.tolist() == [[lin(shape, 4, 5, 11), 1, 0]] and gr[:, 2].tolist() == [0, 0]


def test_empty_masks_have_no_rows():
    z = np.zeros((3, 4, 5), np.uint8)
    pr, gr = ref_table(z, z)
    assert pr.shape == (0, 3) and gr.shape == (0, 3)
    pr, gr = ref_table(z, np.ones_like(z))
    assert pr.shape == (0, 3) and gr.tolist() == [[0, 60, 0]]


def test_ref_rows_of_a_random_mask_add_up():
    rng = np.random.default_rng(0)
    a, b = rng.random((9, 10, 11)) < 0.3, rng.random((9, 10, 11)) < 0.3
    for conn in (6, 26):
        ra, rb = ref_table(a, b, conn)
        assert ra[:, 1].sum() == a.sum() and rb[:, 1].sum() == b.sum()
        assert ra[:, 2].sum() == rb[:, 2].sum() == (a & b).sum()
        assert (np.diff(ra[:, 0]) > 0).all() and a.reshape(-1)[ra[:, 0]].all()


# ---- lesions.csv and the summary ----------------------------------------------------------------------------------
def _results(spacing=None):
    """Two subjects, two classes; rows d, h, w, size, overlap."""
    t = lambda rows: np.array(rows, np.int64).reshape(-1, 5)
    res = [{"name": "s1", "counts": torch.zeros(2, 4),
            "lesion_table": [(t([[0, 1, 2, 5, 0], [3, 0, 0, 120, 7]]), t([[3, 0, 1, 30, 7]])),
                             (t([]), t([[9, 9, 9, 1, 0]]))]},
           {"name": "s2", "counts": torch.zeros(2, 4),
            "lesion_table": [(t([[1, 1, 1, 9, 9], [2, 2, 2, 10, 1], [4, 4, 4, 999, 0], [5, 5, 5, 1000, 3]]), t([])),
                             (t([[0, 0, 0, 4000, 0]]), t([]))]}]
    if spacing is not None:
        for r in res:
            r["spacing"] = spacing
    return res


def test_lesions_csv_has_one_row_per_lesion_in_the_documented_order(tmp_path):
    path = str(tmp_path / "lesions.csv")
    E.write_lesions_csv(path, _results())
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["subject", "class", "kind", "lesion", "d", "h", "w", "size", "overlap"]
    assert rows[1:5] == [["s1", "0", "label", "1", "0", "1", "2", "5", "0"],
                         ["s1", "0", "label", "2", "3", "0", "0", "120", "7"],
                         ["s1", "0", "pred", "1", "3", "0", "1", "30", "7"],
                         ["s1", "1", "pred", "1", "9", "9", "9", "1", "0"]]
    assert len(rows) == 1 + 4 + 5 and rows[-1] == ["s2", "1", "label", "1", "0", "0", "0", "4000", "0"]


def test_lesions_csv_adds_the_volume_only_with_a_spacing_and_never_mixes(tmp_path):
    path = str(tmp_path / "lesions.csv")
    E.write_lesions_csv(path, _results((2.5, 0.9, 0.9)))
    rows = list(csv.reader(open(path)))
    assert rows[0][-2:] == ["overlap", "vol_mm3"] and len(rows[0]) == 10
    assert rows[1][-1] == "%.7g" % (5 * 2.5 * 0.9 * 0.9) and rows[2][-1] == "%.7g" % (120 * 2.5 * 0.9 * 0.9)
    mixed = _results()
    mixed[1]["spacing"] = (1.0, 1.0, 1.0)
    with pytest.raises(RuntimeError):
        E.write_lesions_csv(path, mixed)


def test_lesion_size_summary_bins_the_label_lesions():
    assert E.LESION_SIZE_BINS == ((1, 9), (10, 99), (100, 999), (1000, None))
    got = E.lesion_size_summary(_results())
    assert got.dtype == np.int64 and got.shape == (2, 4, 2)
    # class 0: sizes 5 (missed), 120 (hit), 9 (hit), 10 (hit), 999 (missed), 1000 (hit); class 1: 4000 (missed)
    assert got[0].tolist() == [[2, 1], [1, 1], [2, 1], [1, 1]]
    assert got[1].tolist() == [[0, 0], [0, 0], [0, 0], [1, 0]]
