"""Lesion-level validation metrics (--is_cc), host side (no GPU): the flag and its YAML key, the C-ABI rows of the
connected-component kernels, the lesion columns of metrics.csv, and the yardstick the GPU tests compare against - a
small numpy labeller and a restatement of the reference's num_component / num_false_positive / num_positive /
num_false_negative (utils/metrics.py:69-94) with the 3 x 3 x 3 neighbourhood - on hand-made cases with known answers."""
import csv
import os
import re

import numpy as np
import torch

from efficientq_amd import _lib, config as Cf, evaluate as E

try:
    from scipy import ndimage
except ImportError:          # the extra assertions against scipy are then not made
    ndimage = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the yardstick ------------------------------------------------------------------------------------------------
def ref_label(mask, connectivity=26):
    """Labels of a D x H x W mask: 0 for background, else 1 + the least linear index of the voxel's component.  Every
    foreground voxel starts at 1 + its own index and takes the minimum over its neighbourhood until nothing changes; in
    between it also takes the label of the voxel its label names (a voxel of the same component whose label cannot be
    below the component's least index), which only shortens long paths."""
    m = np.asarray(mask) != 0
    assert m.ndim == 3 and connectivity in (6, 26)
    D, H, W = m.shape
    big = np.int64(m.size + 1)
    offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)
            if (a, b, c) != (0, 0, 0) and (connectivity == 26 or abs(a) + abs(b) + abs(c) == 1)]
    lab = np.where(m, np.arange(1, m.size + 1, dtype=np.int64).reshape(m.shape), big)
    fg = m.reshape(-1)
    while True:
        pad = np.pad(lab, 1, constant_values=big)
        new = lab.copy()
        for a, b, c in offs:
            new = np.minimum(new, pad[1 + a:1 + a + D, 1 + b:1 + b + H, 1 + c:1 + c + W])
        new = np.where(m, new, big)
        flat = new.reshape(-1)
        for _ in range(3):
            flat[fg] = flat[flat[fg] - 1]
        if np.array_equal(new, lab):
            break
        lab = new
    out = np.where(m, lab, 0).astype(np.int32)
    if ndimage is not None:      # numbered in raster order of the first voxel this is scipy's labelling
        want, n = ndimage.label(m, np.ones((3, 3, 3)) if connectivity == 26 else None)
        ids = np.unique(out[out > 0])
        assert n == len(ids)
        assert np.array_equal(np.where(m, np.searchsorted(ids, out) + 1, 0), want)
    return out


def num_components(labels):
    return len(np.unique(labels[labels > 0]))


def num_missed(a_labels, b_mask):
    """metrics.num_false_positive(a, b): the components of a that hold no voxel of b."""
    every = np.unique(a_labels[a_labels > 0])
    hit = np.unique(a_labels[(a_labels > 0) & (np.asarray(b_mask) != 0)])
    return len(every) - len(hit)


def lesion_counts(pred, gt, connectivity=26):
    """[totall, predl, fnl, fpl] of one class: num_positive = num_component(target), the components of the prediction,
    num_false_negative = num_false_positive(target, pred), num_false_positive(pred, target)."""
    pl, gl = ref_label(pred, connectivity), ref_label(gt, connectivity)
    return [num_components(gl), num_components(pl), num_missed(gl, pred), num_missed(pl, gt)]


# ---- the flag -----------------------------------------------------------------------------------------------------
def test_parser_knows_is_cc_and_a_yaml_key_sets_it(tmp_path):
    assert Cf.build_parser().parse_args(["ptq"]).is_cc is False
    assert Cf.build_parser().parse_args(["ptq", "--is_cc"]).is_cc is True
    assert Cf.make_args(Cf.TINY_NET, 4, 4).is_cc is False
    cfg = tmp_path / "cc.yaml"
    cfg.write_text("is_cc: true\ntask: lits\n")
    args = Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["ptq"]))
    assert args.is_cc is True and args.task == "lits"


def test_component_symbols_in_header_and_signatures():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("effq_cc_label", "effq_seg_lesions"):
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    assert re.search(r"\bsize_t effq_cc_ws_bytes\s*\(\s*int P, int D, int H, int W\s*\)", hdr)
    assert "effq_cc_ws_bytes" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["effq_cc_label"][1]) == 11 and len(_lib.SIGNATURES["effq_seg_lesions"][1]) == 14
    assert _lib.LESION_CONNECTIVITY == 26


def test_kernels_take_their_decisions_from_the_shared_header():
    csrc = os.path.join(ROOT, "efficientq_amd", "csrc")
    assert "void decide(" in open(os.path.join(csrc, "seg_decide.h")).read()
    for name in ("seg_eval.hip", "seg_cc.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "seg_decide.h"' in text and "void decide(" not in text, name
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "seg_cc.hip" in mk and "seg_decide.h" in mk


# ---- metrics.csv --------------------------------------------------------------------------------------------------
def _results(with_lesions):
    res = []
    for name, counts, les in (("s1", [[3, 1, 2, 4], [1, 0, 0, 9]], [[2, 3, 1, 2], [1, 1, 0, 0]]),
                              ("s2", [[0, 2, 0, 8], [5, 0, 5, 0]], [[0, 4, 0, 4], [7, 5, 3, 1]])):
        r = {"name": name, "counts": torch.tensor(counts)}
        r.update(E.metrics_from_counts(r["counts"]))
        if with_lesions:
            r["lesions"] = torch.tensor(les)
        res.append(r)
    return res


def test_metrics_csv_appends_the_lesion_columns_only_when_present(tmp_path):
    plain, cc = str(tmp_path / "plain.csv"), str(tmp_path / "cc.csv")
    E.write_metrics_csv(plain, _results(False))
    E.write_metrics_csv(cc, _results(True))
    head = ["subject", "class", "dsc", "sens", "spec", "acc", "tp", "fp", "fn", "tn"]
    rows_plain, rows_cc = list(csv.reader(open(plain))), list(csv.reader(open(cc)))
    assert rows_plain[0] == head
    assert rows_cc[0] == head + ["totall", "predl", "fnl", "fpl"] == head + list(E.LESION_COLUMNS)
    assert [r[:10] for r in rows_cc] == rows_plain
    assert [r[10:] for r in rows_cc[1:]] == [["2", "3", "1", "2"], ["1", "1", "0", "0"], ["0", "4", "0", "4"],
                                              ["7", "5", "3", "1"]]


def test_lesion_totals_sum_per_class():
    tot = E.lesion_totals(_results(True))
    assert tot.dtype == torch.int64 and tot.tolist() == [[2, 7, 1, 6], [8, 6, 3, 1]]


# ---- the labeller and the restatement on hand-made cases ----------------------------------------------------------
def test_blobs_touching_at_a_corner_are_one_component_at_26_and_two_at_6():
    m = np.zeros((6, 7, 8), np.uint8)
    m[1:3, 1:3, 1:3] = 1
    m[3:5, 3:5, 3:5] = 1                      # (2, 2, 2) and (3, 3, 3) share a corner only
    first = (1 * 7 + 1) * 8 + 1
    l26, l6 = ref_label(m, 26), ref_label(m, 6)
    assert num_components(l26) == 1 and set(np.unique(l26)) == {0, 1 + first}
    assert num_components(l6) == 2 and set(np.unique(l6)) == {0, 1 + first, 1 + (3 * 7 + 3) * 8 + 3}
    assert np.array_equal(l26 > 0, m > 0) and np.array_equal(l6 > 0, m > 0)
    # an edge contact is a contact at 26 only, too
    e = np.zeros((4, 4, 4), np.uint8)
    e[0, 0, :] = 1
    e[1, 1, :] = 1
    assert num_components(ref_label(e, 26)) == 1 and num_components(ref_label(e, 6)) == 2


def test_a_predicted_blob_over_two_label_blobs():
    gt = np.zeros((5, 6, 12), np.uint8)
    gt[1:3, 1:3, 1:3] = 1
    gt[1:3, 1:3, 8:10] = 1
    pred = np.zeros_like(gt)
    pred[2, 2, 2:9] = 1                       # one bar through both
    assert lesion_counts(pred, gt) == [2, 1, 0, 0]
    assert lesion_counts(gt, pred) == [1, 2, 0, 0]
    pred[4, 5, 11] = 1                        # a false lesion
    assert lesion_counts(pred, gt) == [2, 2, 0, 1]
    pred[2, 2, 2:9] = 0                       # the bar gone: both labelled lesions missed
    assert lesion_counts(pred, gt) == [2, 1, 2, 1]


def test_empty_masks_have_no_lesions():
    z = np.zeros((3, 4, 5), np.uint8)
    assert lesion_counts(z, z) == [0, 0, 0, 0]
    assert not ref_label(z).any()
    one = np.ones_like(z)
    assert lesion_counts(z, one) == [1, 0, 1, 0] and lesion_counts(one, z) == [0, 1, 0, 1]


def test_labeller_follows_a_long_path():
    m = np.zeros((1, 9, 40), np.uint8)        # a serpentine: the least index has to travel its whole length
    for h in range(0, 9, 2):
        m[0, h, :] = 1
    for k, h in enumerate(range(1, 9, 2)):
        m[0, h, 39 if k % 2 == 0 else 0] = 1
    for conn in (6, 26):
        lab = ref_label(m, conn)
        assert np.array_equal(lab, m.astype(np.int32))      # one component, first voxel 0
