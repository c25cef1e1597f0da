"""Surface-distance validation metrics (--surf_dist), host side (no GPU): the yardstick the GPU tests compare against -
the 6-neighbour surface, a brute-force exact squared distance map and hd / hd95 / assd from the two sorted distance lists
in numpy fp64 - on hand-made cases with known answers; evaluate.surface_metrics from hand-written device outputs; the
flag and its YAML key, the C-ABI rows of the distance-transform kernels and the surface columns of metrics.csv.
All distances are in voxel units."""
import csv
import math
import os
import re

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, evaluate as E

try:
    from scipy import ndimage
except ImportError:          # the extra assertions against scipy are then not made
    ndimage = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.iinfo(np.int32).max


# ---- the yardstick ------------------------------------------------------------------------------------------------
def ref_surface(mask):
    """S(M): the voxels of M with a face neighbour that is background, everything outside the volume being background."""
    m = np.asarray(mask) != 0
    assert m.ndim == 3
    pad = np.pad(m, 1, constant_values=False)
    inner = m.copy()
    for ax in range(3):
        for step in (-1, 1):
            inner &= np.roll(pad, step, ax)[1:-1, 1:-1, 1:-1]
    out = m & ~inner
    if ndimage is not None:
        assert np.array_equal(out, m & ~ndimage.binary_erosion(m, ndimage.generate_binary_structure(3, 1)))
    return out


def ref_edt_sq(sites):
    """E(v) = min over the sites s of |v - s|^2 by brute force in int64 (small volumes); INT32_MAX without a site."""
    s = np.asarray(sites) != 0
    assert s.ndim == 3
    pts = np.argwhere(s).astype(np.int64)
    if len(pts) == 0:
        return np.full(s.shape, INF, np.int64)
    vox = np.indices(s.shape).reshape(3, -1).T.astype(np.int64)
    best = np.full(len(vox), np.iinfo(np.int64).max)
    for k in range(0, len(pts), 256):
        d = ((vox[:, None, :] - pts[None, k:k + 256, :]) ** 2).sum(-1)
        best = np.minimum(best, d.min(1))
    out = best.reshape(s.shape)
    if ndimage is not None:
        assert np.array_equal(out, np.rint(ndimage.distance_transform_edt(~s) ** 2).astype(np.int64))
    return out


def edt_sq_lines(sites):
    """The same map for volumes too large for the brute force: exact in int64 axis by axis, min_j (g(j) + (i - j)^2)
    over whole lines.  scipy, when it imports, is asserted to agree."""
    s = np.asarray(sites) != 0
    big = np.int64(1) << 40
    g = np.where(s, np.int64(0), big)
    for ax in range(3):
        n = s.shape[ax]
        g = np.moveaxis(g, ax, 0)
        i = np.arange(n, dtype=np.int64)
        out = np.full_like(g, big)
        for j in range(n):
            out = np.minimum(out, g[j][None] + ((i - j) ** 2).reshape((n,) + (1,) * (g.ndim - 1)))
        g = np.moveaxis(out, 0, ax)
    g = np.where(g >= big, np.int64(INF), g)
    if ndimage is not None and s.any():
        assert np.array_equal(g, np.rint(ndimage.distance_transform_edt(~s) ** 2).astype(np.int64))
    return g


def ref_surface_counts(pred, gt, edt=ref_edt_sq):
    """What effq_seg_surface returns for one class: ([nP, nL, maxsq_PL, maxsq_LP, qlo_sq, qhi_sq], [sum_PL, sum_LP])."""
    sp, sl = ref_surface(pred), ref_surface(gt)
    n_p, n_l = int(sp.sum()), int(sl.sum())
    e_pl = np.sort(edt(sl)[sp]) if n_l else np.zeros(0, np.int64)       # E_L over S(P)
    e_lp = np.sort(edt(sp)[sl]) if n_p else np.zeros(0, np.int64)       # E_P over S(L)
    row = [n_p, n_l, int(e_pl.max()) if len(e_pl) else 0, int(e_lp.max()) if len(e_lp) else 0, 0, 0]
    if n_p and n_l:
        pooled = np.sort(np.hstack([e_pl, e_lp]))
        n = len(pooled)
        lo = 95 * (n - 1) // 100
        row[4:] = [int(pooled[lo]), int(pooled[min(lo + 1, n - 1)])]
    return row, [float(np.sqrt(e_pl.astype(np.float64)).sum()), float(np.sqrt(e_lp.astype(np.float64)).sum())]


def ref_surface_metrics(pred, gt, edt=ref_edt_sq):
    """(hd, hd95, assd) of one class from the definitions: medpy's on non-empty masks, 0 when both surfaces are empty,
    sqrt(D^2 + H^2 + W^2) when one is."""
    sp, sl = ref_surface(pred), ref_surface(gt)
    if not sp.any() and not sl.any():
        return (0.0, 0.0, 0.0)
    if not sp.any() or not sl.any():
        return (math.sqrt(sum(e * e for e in sp.shape)),) * 3
    d_pl = np.sqrt(edt(sl)[sp].astype(np.float64))
    d_lp = np.sqrt(edt(sp)[sl].astype(np.float64))
    pooled = np.hstack([d_pl, d_lp])
    return (float(pooled.max()), float(np.percentile(pooled, 95)), float((d_pl.mean() + d_lp.mean()) / 2))


def _metrics_via_host(pred, gt):
    """evaluate.surface_metrics fed with the yardstick's own counts and sums."""
    row, sums = ref_surface_counts(pred, gt)
    return E.surface_metrics(torch.tensor([row]), torch.tensor([sums], dtype=torch.float64), np.shape(pred))[0].tolist()


def _close(got, want, rel=1e-12):
    return all(abs(g - w) <= rel * max(abs(w), 1e-300) for g, w in zip(got, want))


def _box(shape, lo, hi):
    m = np.zeros(shape, np.uint8)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    return m


# ---- the yardstick on hand-made cases -----------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.02, 0.3])
def test_brute_force_and_line_maps_agree_on_random_sites(density):
    s = np.random.default_rng(3).random((11, 13, 17)) < density
    assert np.array_equal(ref_edt_sq(s), edt_sq_lines(s))
    assert (ref_edt_sq(s)[s] == 0).all()
    assert (edt_sq_lines(np.zeros((3, 4, 5))) == INF).all() and (ref_edt_sq(np.zeros((3, 4, 5))) == INF).all()


def test_concentric_boxes_have_closed_form_distances():
    shape = (14, 15, 16)
    outer, inner = _box(shape, (2, 2, 2), (12, 12, 12)), _box(shape, (4, 4, 4), (10, 10, 10))
    so, si = ref_surface(outer), ref_surface(inner)
    assert so.sum() == 10 ** 3 - 8 ** 3 and si.sum() == 6 ** 3 - 4 ** 3
    # from the inner surface the outer one is 2 away everywhere; from an outer surface voxel the nearest voxel of the
    # inner box is the voxel clamped into it
    assert (ref_edt_sq(so)[si] == 4).all()
    v = np.argwhere(so)
    want = ((v - np.clip(v, 4, 9)) ** 2).sum(1)
    assert np.array_equal(ref_edt_sq(si)[so], want) and want.max() == 12 and want.min() == 4
    hd, hd95, assd = ref_surface_metrics(outer, inner)
    assert hd == math.sqrt(12)
    assert assd == (np.sqrt(want).mean() + 2.0) / 2
    assert _close(_metrics_via_host(outer, inner), (hd, hd95, assd))
    row, _ = ref_surface_counts(outer, inner)
    assert row[:4] == [488, 152, 12, 4]


def test_a_box_shifted_by_3_4_0_is_5_away():
    shape = (16, 18, 12)
    a, b = _box(shape, (2, 2, 2), (9, 9, 9)), _box(shape, (5, 6, 2), (12, 13, 9))
    hd, hd95, assd = ref_surface_metrics(a, b)
    assert hd == 5.0 and 0 < assd < hd95 <= hd
    assert ref_surface_metrics(b, a) == (hd, hd95, assd)
    assert _close(_metrics_via_host(a, b), (hd, hd95, assd))


def test_single_voxels_at_opposite_corners():
    shape = (5, 7, 9)
    a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    a[0, 0, 0] = 1
    b[-1, -1, -1] = 1
    want = math.sqrt(4 ** 2 + 6 ** 2 + 8 ** 2)
    assert ref_surface_metrics(a, b) == (want, want, want)
    assert _metrics_via_host(a, b) == [want, want, want]
    assert ref_surface_counts(a, b) == ([1, 1, 116, 116, 116, 116], [want, want])
    assert ref_edt_sq(a)[-1, -1, -1] == 116 and ref_edt_sq(a).max() == 116


def test_the_surface_of_a_full_volume_is_its_shell():
    shape = (5, 6, 7)
    full = np.ones(shape, np.uint8)
    s = ref_surface(full)
    assert s.sum() == 5 * 6 * 7 - 3 * 4 * 5 and not s[1:-1, 1:-1, 1:-1].any() and s[0].all() and s[:, :, -1].all()
    assert ref_surface_metrics(full, full) == (0.0, 0.0, 0.0)
    thin = np.ones((1, 4, 4), np.uint8)               # every voxel of a one-voxel-thick volume is on its border
    assert ref_surface(thin).all()


def test_empty_masks_follow_the_convention():
    shape = (155, 240, 240)
    z = np.zeros((4, 5, 6), np.uint8)
    one = _box((4, 5, 6), (1, 1, 1), (3, 3, 3))
    diag = math.sqrt(16 + 25 + 36)
    assert ref_surface_metrics(z, z) == (0.0, 0.0, 0.0)
    assert ref_surface_metrics(z, one) == ref_surface_metrics(one, z) == (diag, diag, diag)
    assert _metrics_via_host(z, z) == [0.0, 0.0, 0.0]
    assert _metrics_via_host(z, one) == _metrics_via_host(one, z) == [diag, diag, diag]
    assert ref_surface_counts(one, z) == ([8, 0, 0, 0, 0, 0], [0.0, 0.0])
    got = E.surface_metrics(torch.tensor([[0, 7, 0, 0, 0, 0]]), torch.zeros(1, 2, dtype=torch.float64), shape)
    assert round(float(got[0, 1]), 2) == 373.13 and got.dtype == torch.float64 and got.shape == (1, 3)


@pytest.mark.parametrize("k", [20, 21, 40, 7])
def test_pooled_percentile_on_and_off_an_order_statistic(k):
    """k isolated voxels at growing distances from a single voxel: n = k + 1 pooled values; 95 (n - 1) is a multiple of
    100 for k = 20 and k = 40 and is not for the others."""
    shape = (3, 90, 8)
    one = np.zeros(shape, np.uint8)
    one[1, 0, 0] = 1
    many = np.zeros(shape, np.uint8)
    for i in range(k):
        many[1, 2 * i + 3, 3 * i % 8] = 1
    row, sums = ref_surface_counts(many, one)
    n = row[0] + row[1]
    assert n == k + 1 and (95 * (n - 1) % 100 == 0) == (k in (20, 40))
    want = ref_surface_metrics(many, one)
    got = E.surface_metrics(torch.tensor([row]), torch.tensor([sums], dtype=torch.float64), shape)[0].tolist()
    assert _close(got, want)
    assert row[4] <= row[5] <= max(row[2], row[3])


def test_surface_metrics_from_hand_written_counts():
    # class 0: n = 21 pooled values, rank 19 exactly: hd95 = sqrt(qlo); class 1: n = 4, 95 * 3 = 285: between ranks 2, 3
    counts = torch.tensor([[11, 10, 49, 25, 16, 36], [2, 2, 9, 4, 4, 9], [0, 0, 0, 0, 0, 0], [5, 0, 0, 0, 0, 0]])
    sums = torch.tensor([[22.0, 10.0], [4.0, 3.0], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64)
    got = E.surface_metrics(counts, sums, (3, 4, 12))
    assert got.dtype == torch.float64 and got.shape == (4, 3)
    assert got[0].tolist() == [7.0, 4.0, 1.5]
    assert got[1].tolist() == [3.0, 2.0 + 1.0 * 85 / 100, (2.0 + 1.5) / 2]
    assert got[2].tolist() == [0.0, 0.0, 0.0]
    assert got[3].tolist() == [13.0, 13.0, 13.0]
    assert E.SURFACE_COLUMNS == ("hd", "hd95", "assd")


# ---- the flag -----------------------------------------------------------------------------------------------------
def test_parser_knows_surf_dist_and_a_yaml_key_sets_it(tmp_path):
    assert Cf.build_parser().parse_args(["ptq"]).surf_dist is False
    assert Cf.build_parser().parse_args(["ptq", "--surf_dist"]).surf_dist is True
    both = Cf.build_parser().parse_args(["ptq", "--surf_dist", "--is_cc", "--save_nii"])
    assert both.surf_dist and both.is_cc and both.save_nii
    assert Cf.make_args(Cf.TINY_NET, 4, 4).surf_dist is False
    cfg = tmp_path / "sd.yaml"
    cfg.write_text("surf_dist: true\ntask: brats\n")
    args = Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["ptq"]))
    assert args.surf_dist is True and args.is_cc is False and args.task == "brats"


def test_the_tester_gets_the_switch_only_when_it_is_set():
    """calibrate.do_ptq hands is_surf to the tester like is_cc: not at all unless the flag is set."""
    src = open(os.path.join(ROOT, "efficientq_amd", "calibrate.py")).read()
    assert "cc['is_surf'] = True" in src and "getattr(args, 'surf_dist', False)" in src
    import inspect
    from efficientq_amd import entrance
    sig = inspect.signature(entrance._ValidationTester.test_as_is)
    assert sig.parameters["is_surf"].default is False
    assert inspect.signature(E.validate_seg).parameters["surface"].default is False


def test_surface_symbols_in_header_and_signatures():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("effq_surf_ws_bytes", 4), ("effq_edt_sq", 9), ("effq_seg_surface", 14)):
        m = re.search(rf"\b(?:int|size_t) {name}\s*\(([^)]*)\)", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"\bsize_t effq_surf_ws_bytes\s*\(\s*int P, int D, int H, int W\s*\)", hdr)
    assert int(re.search(r"#define EFFQ_EDT_MAX_LINE (\d+)", hdr).group(1)) == _lib.EDT_MAX_LINE


def test_surface_kernels_take_their_decisions_from_the_shared_header():
    csrc = os.path.join(ROOT, "efficientq_amd", "csrc")
    text = open(os.path.join(csrc, "seg_surface.hip")).read()
    assert '#include "seg_decide.h"' in text and "void decide(" not in text
    assert "void decide(" not in open(os.path.join(csrc, "seg_masks.h")).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "seg_surface.hip" in mk and "seg_masks.h" in mk
    # the passes live in seg_surf.h, written over a metric: the integer file takes EdtVox only, and neither EdtVox nor
    # the shared passes name a floating type
    shared = open(os.path.join(csrc, "seg_surf.h")).read()
    assert "edt_run<EdtVox>" in text and "EdtMm" not in text and "seg_surf.h" in mk
    vox = shared[shared.index("struct EdtVox"):shared.index("struct EdtMm")]
    for part in (vox[:vox.rindex("};")], shared[shared.index("// ---- rows"):]):
        assert not re.search(r"\b(float|double)\b", part), "no float enters the squared distance map"


# ---- metrics.csv --------------------------------------------------------------------------------------------------
def _results(with_lesions, with_surface):
    res = []
    for name, counts, les, sd in (
            ("s1", [[3, 1, 2, 4], [1, 0, 0, 9]], [[2, 3, 1, 2], [1, 1, 0, 0]], [[5.0, 4.25, 1.0 / 3], [0.0, 0.0, 0.0]]),
            ("s2", [[0, 2, 0, 8], [5, 0, 5, 0]], [[0, 4, 0, 4], [7, 5, 3, 1]],
             [[math.sqrt(139225), 373.1286641, 1e-3], [1.0, 1.0, 1.0]])):
        r = {"name": name, "counts": torch.tensor(counts)}
        r.update(E.metrics_from_counts(r["counts"]))
        if with_lesions:
            r["lesions"] = torch.tensor(les)
        if with_surface:
            r["surface"] = torch.tensor(sd, dtype=torch.float64)
            r["surface_counts"] = torch.zeros(2, 6, dtype=torch.int64)
        res.append(r)
    return res


@pytest.mark.parametrize("with_lesions", [False, True])
def test_metrics_csv_appends_the_surface_columns_only_when_present(tmp_path, with_lesions):
    plain, sd = str(tmp_path / "plain.csv"), str(tmp_path / "sd.csv")
    E.write_metrics_csv(plain, _results(with_lesions, False))
    E.write_metrics_csv(sd, _results(with_lesions, True))
    head = ["subject", "class", "dsc", "sens", "spec", "acc", "tp", "fp", "fn", "tn"]
    head += ["totall", "predl", "fnl", "fpl"] if with_lesions else []
    bytes_plain = open(plain, "rb").read()
    rows_plain, rows_sd = list(csv.reader(open(plain))), list(csv.reader(open(sd)))
    assert rows_plain[0] == head
    assert rows_sd[0] == head + ["hd", "hd95", "assd"] == head + list(E.SURFACE_COLUMNS)
    k = len(head)
    assert [r[:k] for r in rows_sd] == rows_plain
    # the other columns byte for byte: dropping the three fields of every line gives the plain file back
    stripped = b"".join(b",".join(line.split(b",")[:k]) + b"\r\n" for line in open(sd, "rb").read().splitlines())
    assert stripped == bytes_plain
    assert [r[k:] for r in rows_sd[1:]] == [["5", "4.25", "0.3333333"], ["0", "0", "0"],
                                            ["373.1287", "373.1287", "0.001"], ["1", "1", "1"]]


def test_surface_means_average_per_class():
    m = E.surface_means(_results(False, True))
    assert m.dtype == torch.float64 and m.shape == (2, 3)
    assert m[1].tolist() == [0.5, 0.5, 0.5] and float(m[0, 1]) == (4.25 + 373.1286641) / 2
