"""The `predict` mission, host side (no GPU): the fp64 restatement of effq_seg_labels_source (ref_labels_source, which the
GPU tests compare the kernel with), hand-computed cases of its inverse map and inside test, the parser, what the mission
refuses, the C-ABI row of the new symbol, and the whole mission driven through numpy stand-ins for the device ops."""
import csv
import os
import re

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, evaluate as E, nifti, predict, prep
from tests.test_prep_cpu import NumpyOps, write_scan, written

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------
def ref_axis_source(n_src, f, G, pmin, g):
    """Per source index of one axis: inside, i0, i1 and the fp64 weight of i1.  t = (s + 0.5) / f; inside iff pmin <=
    min(floor(t), G - 1) < pmin + g; q = clamp(t - 0.5 - pmin, 0, g - 1) (the inverse of test_prep_cpu.ref_axis_linear)."""
    t = (np.arange(n_src, dtype=np.float64) + 0.5) / np.float64(f)
    n = np.minimum(np.floor(t), G - 1.0)
    inside = (n >= pmin) & (n < pmin + g)
    q = np.clip(t - 0.5 - pmin, 0.0, g - 1.0)
    i0 = np.floor(q).astype(np.int64)
    return inside, i0, np.minimum(i0 + 1, g - 1), q - i0


def ref_merge(bits, fuse):
    """C x ... bool: agg p[i] = any(p[i:]), con p[i] = all(p[:i+1])."""
    if fuse in ("agg", "aggressive"):
        return np.flip(np.logical_or.accumulate(np.flip(bits, 0), 0), 0)
    if fuse in ("con", "conservative"):
        return np.logical_and.accumulate(bits, 0)
    assert fuse is None
    return bits


def ref_labels_source(logits, pmin, grid, factors, source_shape, rule, fuse=None, thresh=0.0):
    """(labels uint8, margin fp64, inside bool), each of `source_shape`: the rule of effq_seg_labels_source with the
    weights, the interpolation and the decisions in fp64.  margin: how far the fp64 values are from deciding otherwise -
    the gap between the two largest channels for argmax (inf for one channel), min over the channels of |v - thresh|
    for the sigmoid rules; inf outside the box."""
    v = np.asarray(logits, dtype=np.float64)
    C, box = v.shape[0], v.shape[1:]
    f = (1.0, 1.0, 1.0) if factors is None else factors
    (md, d0, d1, ld), (mh, h0, h1, lh), (mw, w0, w1, lw) = (
        ref_axis_source(n, fa, G, lo, g) for n, fa, G, lo, g in zip(source_shape, f, grid, pmin, box))
    inside = md[:, None, None] & mh[None, :, None] & mw[None, None, :]
    ld, lh, lw = ld[:, None, None], lh[None, :, None], lw[None, None, :]
    at = lambda d, h, w: v[:, d[:, None, None], h[None, :, None], w[None, None, :]]
    a = (1 - lh) * ((1 - lw) * at(d0, h0, w0) + lw * at(d0, h0, w1)) + lh * ((1 - lw) * at(d0, h1, w0) + lw * at(d0, h1, w1))
    b = (1 - lh) * ((1 - lw) * at(d1, h0, w0) + lw * at(d1, h0, w1)) + lh * ((1 - lw) * at(d1, h1, w0) + lw * at(d1, h1, w1))
    x = (1 - ld) * a + ld * b                                  # C x source
    if rule == "argmax":
        assert fuse is None
        lab = np.argmax(x, 0)                                   # the first maximum
        top = np.sort(x, 0)
        margin = top[-1] - top[-2] if C > 1 else np.full(x.shape[1:], np.inf)
    else:
        t = np.float64(np.float32(thresh))
        bits = ref_merge(x >= t, fuse)
        margin = np.abs(x - t).min(0)
        if rule == "brats":
            assert C >= 3
            lab = np.zeros(x.shape[1:], dtype=np.int64)
            lab[bits[0]] = 1
            lab[bits[0] & ~bits[1]] = 2
            lab[bits[2]] = 4
        else:
            assert rule == "rank"
            lab = np.where(bits.any(0), C - np.argmax(np.flip(bits, 0), 0), 0)
    return (np.where(inside, lab, 0).astype(np.uint8), np.where(inside, margin, np.inf), inside)


class PredictOps(NumpyOps):
    """NumpyOps with the window ops (evaluate's own torch path) and seg_labels_source through the restatement: for the
    orchestration tests only."""
    THRESH = 0.0

    @staticmethod
    def window_grid(dhw, patch, overlap):
        return tuple(len(E.window_starts(s, p, o)) for s, p, o in zip(dhw, patch, overlap))

    def window_gather(self, vol, patch, overlap, first=0, count=None, flip=0):
        pats = E.image_to_patch3d(vol, patch, overlap)
        pats = pats[first:] if count is None else pats[first:first + count]
        win = torch.cat([pt.permute(0, 2, 3, 4, 1) for pt in pats]).contiguous()
        dims = [1 + b for b in range(3) if flip >> b & 1]
        return torch.flip(win, dims).contiguous() if dims else win

    def window_put(self, last, buf_slice, flip=0, accumulate=False):
        assert buf_slice.is_contiguous()
        dims = [1 + b for b in range(3) if flip >> b & 1]
        v = last.permute(0, 2, 3, 4, 1)
        v = torch.flip(v, dims) if dims else v
        if accumulate:
            buf_slice.add_(v)
        else:
            buf_slice.copy_(v)

    def window_stitch(self, win, shape, patch, overlap, weights=None, nflip=1):
        assert weights is None and nflip == 1       # the blend is tests.test_window_blend_cpu.BlendOps'
        N = int(shape[0])
        pats = [win[i * N:(i + 1) * N].permute(0, 4, 1, 2, 3) for i in range(win.shape[0] // N)]
        return E.patch_to_image3d(torch.empty(tuple(shape)), pats, patch, overlap).contiguous()

    def seg_labels_source(self, logits, pmin, grid, factors, source_shape, rule, fuse=None):
        lab, _, _ = ref_labels_source(logits.numpy(), pmin, grid, factors, source_shape, rule, fuse, self.THRESH)
        return torch.from_numpy(lab)


class PointNet(torch.nn.Module):
    """One modality to three classes, voxel by voxel."""

    def forward(self, x):
        return torch.cat([0.3 - x * x, x - 0.2, -x - 0.4], 1)


# ---- hand-computed axes ----------------------------------------------------------------------------------------------------
def test_inverse_map_and_inside_test_match_hand_computed_cases():
    # f = 1 with a crop: source index s is working voxel s, the box holds 2, 3, 4
    inside, i0, i1, l = ref_axis_source(6, 1.0, 6, 2, 3)
    assert inside.tolist() == [False, False, True, True, True, False]
    assert i0[2:5].tolist() == [0, 1, 2] and i1[2:5].tolist() == [1, 2, 2] and l[2:5].tolist() == [0.0, 0.0, 0.0]
    # f = 0.5: source voxel s covers working voxels 2 s and 2 s + 1; its centre lies half-way between them
    inside, i0, i1, l = ref_axis_source(4, 0.5, 8, 0, 8)
    assert inside.all() and i0.tolist() == [0, 2, 4, 6] and i1.tolist() == [1, 3, 5, 7] and l.tolist() == [0.5] * 4
    # ... and the first and the last source voxel on either side of pmin = 3 and pmax = 5: n = 2 s + 1 = 1, 3, 5, 7
    inside, i0, i1, l = ref_axis_source(4, 0.5, 8, 3, 2)
    assert inside.tolist() == [False, True, False, False]
    assert (i0[1], i1[1], l[1]) == (0, 1, 0.0)                  # t = 3: q = 3 - 0.5 - 3 = -0.5, clamped to 0
    assert (i0[0], l[0], i0[2], l[2]) == (0, 0.0, 1, 0.0)       # outside: clamped to the ends of the box
    # f = 2.5: ten source voxels over four working voxels, t = 0.2, 0.6, 1.0, 1.4, 1.8, 2.2, 2.6, 3.0, 3.4, 3.8
    inside, i0, i1, l = ref_axis_source(10, 2.5, 4, 1, 2)
    assert inside.tolist() == [False, False, True, True, True, True, True, False, False, False]
    assert i0[2:7].tolist() == [0, 0, 0, 0, 1] and i1[2:7].tolist() == [1, 1, 1, 1, 1]
    assert l[2:7] == pytest.approx([0.0, 0.0, 0.3, 0.7, 0.0], abs=1e-12)
    # floor(t) = G is clamped in: three source voxels at f = 2.5 make a grid of round(1.2) = 1; t(2) = 2.5 / 2.5 = 1 = G
    assert prep.resample_extent(3, 2.5) == 1
    inside, i0, i1, l = ref_axis_source(3, 2.5, 1, 0, 1)
    assert inside.tolist() == [True, True, True] and i0.tolist() == [0, 0, 0] and i1.tolist() == [0, 0, 0]
    # the map inverts prep's: working voxel o lies at source coordinate (o + 0.5) f - 0.5, whose t - 0.5 is o again
    for f in (0.64, 1.37, 2.5):
        o = np.arange(7, dtype=np.float64)
        s = (o + 0.5) * f - 0.5
        assert ((s + 0.5) / f - 0.5) == pytest.approx(o, abs=1e-12)


def test_restatement_decides_and_labels_as_seg_labels_does():
    v = np.zeros((3, 1, 1, 4))
    v[:, 0, 0, 0] = (1.0, 1.0, -0.5)       # channels 1 1 0; a tie of the first two: the first maximum
    v[:, 0, 0, 1] = (-1.0, 2.0, 2.0)       # 0 1 1
    v[:, 0, 0, 2] = (0.0, -1.0, 3.0)       # 1 0 1: 0 >= thresh 0 holds
    v[:, 0, 0, 3] = (1.0, -1.0, -1.0)      # 1 0 0
    args = ((0, 0, 0), (1, 1, 4), None, (1, 1, 4))
    lab, margin, inside = ref_labels_source(v, *args, "argmax")
    assert lab.ravel().tolist() == [0, 1, 2, 0] and margin.ravel().tolist() == [0.0, 0.0, 3.0, 2.0] and inside.all()
    assert ref_labels_source(v, *args, "brats")[0].ravel().tolist() == [1, 4, 4, 2]
    assert ref_labels_source(v, *args, "brats", "agg")[0].ravel().tolist() == [1, 4, 4, 2]
    assert ref_labels_source(v, *args, "brats", "con")[0].ravel().tolist() == [1, 0, 2, 2]
    assert ref_labels_source(v, *args, "rank", "con")[0].ravel().tolist() == [2, 0, 1, 1]
    assert ref_labels_source(v, *args, "rank")[0].ravel().tolist() == [2, 3, 3, 1]
    assert ref_labels_source(v, *args, "rank")[1].ravel().tolist() == [0.5, 1.0, 0.0, 1.0]


# ---- the switches -----------------------------------------------------------------------------------------------------------
def test_parser_knows_the_mission_and_its_switches_and_yaml_sets_them(tmp_path):
    a = Cf.build_parser().parse_args(["predict", "--task", "lits", "--resume", "s/state_in_fp.pkl", "--src_list", "c.csv",
                                      "--out_dir", "seg", "--prep_window", "-200,250", "--patch_size", "32,32,16"])
    assert a.mission == "predict" and a.out_dir == "seg" and a.resume == "s/state_in_fp.pkl" and a.pretrain is None
    assert Cf.build_parser().parse_args(["ptq"]).out_dir is None
    cfg = tmp_path / "p.yaml"
    cfg.write_text("out_dir: elsewhere\nresume: other.pkl\n")
    a = Cf.merge_config(str(cfg), a)
    assert a.out_dir == "elsewhere" and a.resume == "other.pkl"            # YAML beats the command line


def test_header_and_lib_row_of_the_source_labels_have_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = re.findall(r"\bint (effq_seg_labels_source)\s*\((.*?)\)\s*;", code, flags=re.S)
    assert len(found) == 1

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return _lib._P
        return {"int": _lib._I, "float": _lib._F, "double": _lib._D}[decl.split()[0]]
    res, got = _lib.SIGNATURES["effq_seg_labels_source"]
    assert res == _lib._I and got == [ctype(a) for a in found[0][1].split(",")] and len(got) == 12
    assert "seg_source.hip" in open(os.path.join(ROOT, "efficientq_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "efficientq_amd", "csrc", "seg_source.hip")).read()
    assert not re.search(r"atomic\w*\s*\(", re.sub(r"//.*", "", src))       # deterministic: no atomics at all
    assert '#include "seg_decide.h"' in src and "predict<MODE, C>" in src and "label_of<RULE, C>" in src


# ---- synthetic scans ----------------------------------------------------------------------------------------------------------
def ct_like(seed, shape=(20, 24, 28), margin=((2, 3), (4, 1), (3, 5))):
    """An int16 scan with a zero margin of differing width per side and values on both sides of the LiTS window."""
    g = np.random.default_rng(seed)
    vol = np.zeros(shape, dtype=np.int16)
    body = tuple(slice(a, n - b) for (a, b), n in zip(margin, shape))
    vol[body] = g.integers(-400, 500, size=vol[body].shape)
    vol[body][vol[body] == 0] = 7
    return vol, body


def write_cases(root, names, seeds, affine=None, **kw):
    os.makedirs(os.path.join(root, "src"), exist_ok=True)
    rows, truth = [], {}
    for sn, seed in zip(names, seeds):
        vol, body = ct_like(seed, **kw)
        rows.append([sn, os.path.join("src", f"{sn}_ct.nii.gz")])
        write_scan(os.path.join(root, rows[-1][1]), vol, affine=affine)
        truth[sn] = (vol, body)
    with open(os.path.join(root, "cases.csv"), "w") as f:
        f.write("subject,ct\n" + "".join(",".join(r) + "\n" for r in rows))
    return os.path.join(root, "cases.csv"), truth


def predict_args(*extra, **over):
    a = Cf.build_parser().parse_args(["predict", "--task", "lits"] + list(extra))
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_leave_out_dir_empty(tmp_path):
    root, out = str(tmp_path), str(tmp_path / "seg")
    lst, _ = write_cases(root, ["a", "b"], [1, 2])
    snap = tmp_path / "state_in_fp.pkl"
    snap.write_bytes(b"")

    def refused(named, model=None, **over):
        kw = dict(src_list=lst, out_dir=out, patch_size="8,8,8", resume=str(snap))
        kw.update(over)
        with pytest.raises(SystemExit) as e:
            predict.run(predict_args(**kw), ops=PredictOps(), model=model, window_batch=2)
        assert all(n in str(e.value) for n in named), str(e.value)
        assert not os.path.exists(out)
    refused(["--resume", "--pretrain", "neither"], resume=None)
    refused(["--resume", "--pretrain", "both"], pretrain=str(snap))
    refused(["--pretrain", "--qconv conv", "effq"], resume=None, pretrain=str(snap), qconv="effq")
    refused(["--multi_label lits", "plane"], model=PointNet(), multi_label="lits")
    refused(["--prep_min_size", "--patch_size"], model=PointNet(), prep_min_size="4,8,8")
    # a missing scan: the row names it
    with open(os.path.join(root, "gone.csv"), "w") as f:
        f.write("subject,ct\na,src/a_ct.nii.gz\nc,src/c_ct.nii.gz\n")
    refused(["row 3", "subject c", "missing"], model=PointNet(), src_list=os.path.join(root, "gone.csv"))
    # a grid smaller than the patch, with and without resampling
    refused(["subject a", "(20, 24, 28)", "smaller"], model=PointNet(), patch_size="8,32,8")
    refused(["subject a", "(10, 12, 14)", "smaller"], model=PointNet(), patch_size="12,12,12", prep_spacing="2,2,2")


# ---- the whole mission on the host ----------------------------------------------------------------------------------------------
def _expected(ops, model, entry, spacing, patch, mask, wb):
    """The map of one subject from the restatement, on logits that went the mission's own way (process_subject and the
    shared window function)."""
    plan = prep._Plan(dict(entry, seg=None), ("ct",), spacing, patch)
    imgs = {"ct": nifti.read_image(entry["images"]["ct"])[0]}
    y, _, _, pmin, pmax, _, _, _ = prep.process_subject(ops, plan, imgs, None, ("ct",),
                                                        prep.PrepOptions(mask, (-200.0, 250.0), spacing, patch, False))
    outs, nwin, _ = E.stitched_window_logits(ops, [model], torch.from_numpy(y)[None], patch, (4, 4, 4), wb)
    lab, _, inside = ref_labels_source(outs[0][0].numpy(), pmin, plan.grid_shape, plan.factors, plan.source_shape, "argmax")
    return lab, inside, plan, pmin, pmax, nwin


@pytest.mark.parametrize("spacing", [None, "2,2,2.5"])
def test_whole_mission_writes_maps_on_the_source_grid_and_the_table(tmp_path, spacing):
    root, out = str(tmp_path), str(tmp_path / "seg")
    aff = np.array([[0.0, -1.0, 0, 30.0], [1.0, 0.0, 0, -4.0], [0, 0, 2.0, 5.0], [0, 0, 0, 1.0]])   # axes 0, 1 rotated
    lst, truth = write_cases(root, ["s2", "s1"], [3, 4], affine=aff)
    ops, model = PredictOps(), PointNet()
    extra = ["--prep_spacing", spacing] if spacing else []
    rows = predict.run(predict_args(*extra, src_list=lst, out_dir=out, patch_size="8,8,8", prep_mask="nonzero"),
                       ops=ops, model=model, window_batch=3)
    assert [r["subject"] for r in rows] == ["s1", "s2"]
    assert written(out) == ["predict.csv", "s1.nii.gz", "s2.nii.gz"]
    table = list(csv.DictReader(open(os.path.join(out, predict.PREDICT_CSV))))
    assert [r["subject"] for r in table] == ["s1", "s2"] and list(table[0]) == predict.CSV_HEADER
    sp = prep._triple(spacing, "spacing") if spacing else None
    for r, entry in zip(table, prep.read_src_list(lst, "lits")):
        sn = r["subject"]
        want, inside, plan, pmin, pmax, nwin = _expected(ops, model, entry, sp, (8, 8, 8), "nonzero", 3)
        got, h = nifti.read_nifti(os.path.join(out, f"{sn}.nii.gz"))
        assert got.dtype == np.uint8 and got.shape == (20, 24, 28) == truth[sn][0].shape
        assert np.allclose(h["affine"], aff) and h["sform_code"] == 2 and h["qform_code"] == 0
        assert list(h["pixdim"][1:4]) == pytest.approx([1.0, 1.0, 1.0])       # the scan's own pixdim, value for value
        assert np.array_equal(got, want)
        assert 0 < inside.sum() < inside.size and not got[~inside].any() and len(np.unique(got)) == 3
        if spacing is None:           # the box is the body: outside it the map is zero, inside it every class shows
            body = truth[sn][1]
            assert pmin == tuple(s.start for s in body) and pmax == tuple(s.stop for s in body)
            assert r["grid_shape"] == "20 24 28" and r["prep_spacing"] == "none"
        else:
            assert r["grid_shape"] == "10 12 22" and r["prep_spacing"] == "2 2 2.5"
        assert r["source_shape"] == "20 24 28" and r["source_spacing"] == "1 1 2"
        assert r["pmin"] == prep._fmt(pmin) and r["pmax"] == prep._fmt(pmax) and int(r["windows"]) == nwin > 1
        assert (r["prep_mask"], r["prep_window"], r["prep_min_size"], r["patch_size"]) == \
            ("nonzero", "-200 250", "8 8 8", "8 8 8")
        count = np.bincount(got.ravel())
        labels = [int(v) for v in r["labels"].split()]
        assert labels == [v for v in range(len(count)) if count[v]]
        assert [int(v) for v in r["voxels"].split()] == [int(count[v]) for v in labels]
        assert [float(v) for v in r["volume_ml"].split()] == pytest.approx([count[v] * 2.0 / 1000 for v in labels], rel=1e-6)


def test_a_seg_column_is_ignored(tmp_path):
    root, out = str(tmp_path), str(tmp_path / "seg")
    lst, _ = write_cases(root, ["a"], [5])
    with open(lst, "w") as f:
        f.write("subject,ct,seg\na,src/a_ct.nii.gz,src/a_ct.nii.gz\n")       # not a label: it must not be read as one
    rows = predict.run(predict_args(src_list=lst, out_dir=out, patch_size="8", prep_mask="nonzero"), ops=PredictOps(),
                       model=PointNet(), window_batch=1)
    assert len(rows) == 1 and os.path.isfile(os.path.join(out, "a.nii.gz"))


# ---- the FP-checkpoint path --------------------------------------------------------------------------------------------------
def _fp_args(**over):
    a = Cf.make_args(dict(Cf.TINY_NET, qconv="conv"), 4, 4, merge_type=None)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_pretrain_path_loads_folds_and_segments_and_refuses_a_checkpoint_that_does_not_fit(tmp_path, capsys):
    from efficientq_amd import calibrate as K, synth
    root, out = str(tmp_path), str(tmp_path / "seg")
    lst, _ = write_cases(root, ["a"], [6])
    QConv, _, kwQ = Cf.get_conv_class(_fp_args())
    assert QConv is torch.nn.Conv3d
    net = Cf.get_model_cube(_fp_args(), QConv, kwQ)[0]["model"]
    synth.randomise_network(net, 3)
    sd = dict(net.state_dict(), **{"optimizer.step": torch.zeros(1)})       # a training checkpoint carries more
    ckpt = str(tmp_path / "state.pkl")
    torch.save({"state_dict": sd}, ckpt)
    ops = PredictOps()
    kw = dict(src_list=lst, out_dir=out, patch_size="8,8,8", prep_mask="nonzero", pretrain=ckpt)
    rows = predict.run(_fp_args(**kw), ops=ops, window_batch=4)
    said = capsys.readouterr().out
    assert "1 keys of the checkpoint" in said and "optimizer.step" in said
    # the same network put together by hand: loaded, folded as do_ptq folds it, in fp mode
    net.eval()
    K.search_fold_and_remove_bn(net)
    K.set_fp(net)
    assert not [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm3d)]
    entry = prep.read_src_list(lst, "lits")[0]
    want, inside, _, pmin, _, nwin = _expected(ops, net, entry, None, (8, 8, 8), "nonzero", 4)
    got, _ = nifti.read_nifti(os.path.join(out, "a.nii.gz"))
    assert np.array_equal(got, want) and rows[0]["pmin"] == prep._fmt(pmin) and int(rows[0]["windows"]) == nwin
    assert got[inside].any() and len(np.unique(got)) > 1
    # a checkpoint of something else: refused by key before out_dir exists
    out2 = str(tmp_path / "seg2")
    torch.save({"state_dict": {"nothing.weight": torch.zeros(1)}}, ckpt)
    with pytest.raises(SystemExit) as e:
        predict.run(_fp_args(**dict(kw, out_dir=out2)), ops=ops, window_batch=4)
    first = next(iter(Cf.get_model_cube(_fp_args(), QConv, kwQ)[0]["model"].state_dict()))
    assert first in str(e.value) and "nothing.weight" in str(e.value) and "--pretrain" in str(e.value)
    assert not os.path.exists(out2)
    # ... and one whose widths differ
    wide = Cf.get_model_cube(_fp_args(width="16,32,16"), QConv, kwQ)[0]["model"]
    torch.save({"state_dict": wide.state_dict()}, ckpt)
    with pytest.raises(SystemExit) as e:
        predict.run(_fp_args(**dict(kw, out_dir=out2)), ops=ops, window_batch=4)
    assert "shapes differ" in str(e.value) and not os.path.exists(out2)
