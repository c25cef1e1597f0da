"""Gaussian window blending and mirror test-time augmentation, host side (no GPU): the switches and what they refuse,
the axes -> flip-mask mapping, the Gaussian weights against their formula, the fp64 restatement of the whole blend
(ref_blend, which the GPU tests compare the kernels with) pinned on a hand-computed case, the C-ABI rows of the window
symbols, and the `predict` mission through numpy / torch stand-ins for the device ops."""
import csv
import os
import re

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, entrance, evaluate as E, hip_ops, predict
from tests.test_predict_cpu import PointNet, PredictOps, predict_args, write_cases
from tests.test_prep_cpu import written

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------
def ref_unflip(win, flip):
    """A channels-last window batch (M, pd, ph, pw, C) mirrored along the axes of the mask `flip` (its own inverse)."""
    axes = [1 + b for b in range(3) if flip >> b & 1]
    return np.flip(win, axes) if axes else win


def ref_blend(passes, weights, shape, patch, overlap):
    """The blend in fp64.  passes: one array (nwin * N, pd, ph, pw, C) per flip pass, window-major and already
    un-mirrored; weights: the three per-axis vectors; shape: (N, C, D, H, W).  Returns (out, mag, cover), fp64 / fp64 /
    int64: out[n, c, d, h, w] = sum over the covering windows and the passes of w v / (len(passes) * sum of w) with
    w = wd[z] wh[y] ww[x]; mag the same with |v| for v (what the fp32 error bound scales with); cover (D, H, W) the
    number of covering windows."""
    N, C, D, H, W = shape
    p, o = tuple(patch), tuple(overlap)
    wd, wh, ww = (np.asarray(w, dtype=np.float64) for w in weights)
    assert (len(wd), len(wh), len(ww)) == p
    w3 = wd[:, None, None] * wh[None, :, None] * ww[None, None, :]
    ps = [np.asarray(a, dtype=np.float64) for a in passes]
    total, mag = sum(ps), sum(np.abs(a) for a in ps)
    acc, amag = np.zeros((N, C, D, H, W)), np.zeros((N, C, D, H, W))
    wsum, cover = np.zeros((D, H, W)), np.zeros((D, H, W), dtype=np.int64)
    n = 0
    for i in E.window_starts(D, p[0], o[0]):
        for j in E.window_starts(H, p[1], o[1]):
            for k in E.window_starts(W, p[2], o[2]):
                box = (slice(i, i + p[0]), slice(j, j + p[1]), slice(k, k + p[2]))
                blk = slice(n * N, (n + 1) * N)
                acc[(slice(None), slice(None)) + box] += np.moveaxis(total[blk] * w3[None, ..., None], -1, 1)
                amag[(slice(None), slice(None)) + box] += np.moveaxis(mag[blk] * w3[None, ..., None], -1, 1)
                wsum[box] += w3
                cover[box] += 1
                n += 1
    assert n * N == ps[0].shape[0] and cover.min() >= 1
    den = len(ps) * wsum
    return acc / den, amag / den, cover


def blend_bound(mag, cover, passes=1):
    """Twice the fp32 bound of the blend per output: T = cover * passes products accumulated in any order, plus the
    weight product, the weight sum and the division: 2 (T + 4) 2^-24 sum(w |v|) / sum(w)."""
    return 2.0 * (cover * passes + 4) * 2.0 ** -24 * mag


def test_restatement_on_a_hand_computed_row():
    # one row of 4 voxels, windows of 3 with overlap 2: starts 0 and 1; weights 1, 3, 1 along w
    shape, p, o = (1, 1, 1, 1, 4), (1, 1, 3), (0, 0, 2)
    assert E.window_starts(4, 3, 2) == [0, 1]
    win = np.array([[1.0, 2.0, 3.0], [10.0, 20.0, 30.0]]).reshape(2, 1, 1, 3, 1)
    w = ([1.0], [1.0], [1.0, 3.0, 1.0])
    out, mag, cover = ref_blend([win], w, shape, p, o)
    # voxel 0: window 0 only; 1: (3 * 2 + 1 * 10) / 4; 2: (1 * 3 + 3 * 20) / 4; 3: window 1 only
    assert out.ravel().tolist() == [1.0, 4.0, 15.75, 30.0] and cover.ravel().tolist() == [1, 2, 2, 1]
    assert mag.ravel().tolist() == [1.0, 4.0, 15.75, 30.0]
    # uniform weights: the mean over the covering windows, evaluate.patch_to_image3d
    out, _, _ = ref_blend([win], ([1.0], [1.0], [1.0] * 3), shape, p, o)
    assert out.ravel().tolist() == [1.0, 6.0, 11.5, 30.0]
    pats = [torch.from_numpy(win[i:i + 1]).permute(0, 4, 1, 2, 3) for i in range(2)]
    assert E.patch_to_image3d(torch.zeros(shape), pats, p, o).ravel().tolist() == [1.0, 6.0, 11.5, 30.0]
    # a second pass, un-mirrored: the passes are summed and the sum is divided by their number as well
    second = np.array([[3.0, -2.0, 1.0], [0.0, 0.0, 0.0]]).reshape(2, 1, 1, 3, 1)
    out, mag, _ = ref_blend([win, second], w, shape, p, o)
    # voxel 1: (3 * (2 - 2) + 1 * (10 + 0)) / (2 * 4); voxel 2: (1 * (3 + 1) + 3 * 20) / 8
    assert out.ravel().tolist() == [2.0, 1.25, 8.0, 15.0]
    assert mag.ravel().tolist() == [2.0, (3 * 4 + 10) / 8, 8.0, 15.0]
    # un-mirroring: mask 4 mirrors w, mask 1 mirrors d (extent 1: nothing moves)
    assert ref_unflip(win, 4)[:, 0, 0, :, 0].tolist() == [[3.0, 2.0, 1.0], [30.0, 20.0, 10.0]]
    assert np.array_equal(ref_unflip(win, 1), win) and ref_unflip(win, 0) is win
    assert blend_bound(np.array([8.0]), np.array([2]), 4)[0] == 2 * 12 * 2.0 ** -24 * 8.0


# ---- the switches -----------------------------------------------------------------------------------------------------------
def test_axes_map_to_every_subset_of_flip_masks():
    assert E.mirror_flips(None) == (0,)
    assert E.mirror_flips("d") == (0, 1) and E.mirror_flips("h") == (0, 2) and E.mirror_flips("w") == (0, 4)
    assert E.mirror_flips("hw") == (0, 2, 4, 6) == E.mirror_flips("wh")
    assert E.mirror_flips("dw") == (0, 1, 4, 5) and E.mirror_flips("dh") == (0, 1, 2, 3)
    assert E.mirror_flips("dhw") == tuple(range(8)) == E.mirror_flips("wdh")
    for bad in ("", "x", "dd", "hwh", "D", "d,h", 3, ("d",)):
        with pytest.raises(ValueError):
            E.mirror_flips(bad)
    assert E.check_flips([0, 4]) == (0, 4)
    for bad in ((), (4, 0), (0, 0), (0, 8), (-1,), (0.0,), (True,)):
        with pytest.raises(ValueError):
            E.check_flips(bad)


def test_parser_defaults_yaml_keys_and_refusals(tmp_path):
    for mission in ("ptq", "predict", "prep"):
        a = Cf.build_parser().parse_args([mission])
        assert a.blend == "uniform" and a.tta_mirror is None
        assert Cf.blend_switches(a) == ("uniform", (0,))
    a = Cf.build_parser().parse_args(["ptq", "--blend", "gauss", "--tta_mirror", "hw"])
    assert Cf.blend_switches(a) == ("gauss", (0, 2, 4, 6))
    cfg = tmp_path / "p.yaml"
    cfg.write_text("blend: gauss\ntta_mirror: dw\n")
    a = Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["predict"]))
    assert Cf.blend_switches(a) == ("gauss", (0, 1, 4, 5))
    cfg.write_text("blend: cosine\n")
    with pytest.raises(SystemExit) as e:
        Cf.blend_switches(Cf.merge_config(str(cfg), Cf.build_parser().parse_args(["predict"])))
    assert "--blend" in str(e.value) and "cosine" in str(e.value)
    # an args object from before the switches (config.make_args) means the defaults
    assert Cf.blend_switches(Cf.make_args(Cf.TINY_NET, 4, 4)) == ("uniform", (0,))

    def refused(argv, named):
        a = Cf.build_parser().parse_args(argv)
        for check in (Cf.blend_switches, entrance.check_switches):
            with pytest.raises(SystemExit) as e:
                check(a)
            assert all(n in str(e.value) for n in named), str(e.value)
    refused(["ptq", "--tta_mirror", "x"], ["--tta_mirror", "'x'"])
    refused(["ptq", "--tta_mirror", "dd"], ["--tta_mirror", "'dd'"])
    refused(["ptq", "--tta_mirror", ""], ["--tta_mirror", "''"])
    refused(["ptq", "--tta_mirror", "dhwd"], ["--tta_mirror"])
    refused(["ptq", "--blend", "cosine"], ["--blend", "cosine", "uniform", "gauss"])
    refused(["ptq", "--blend", ""], ["--blend"])


def test_the_ptq_mission_refuses_before_the_device_and_prep_ignores_the_switches(tmp_path):
    with pytest.raises(SystemExit) as e:
        entrance.main(["ptq", "--task", "lits", "--synthetic", "--snap_dir", str(tmp_path / "snap"), "--tta_mirror", "q"])
    assert "--tta_mirror" in str(e.value) and not os.path.exists(tmp_path / "snap")
    # prep never looks at them: it fails on its own switches, not on these
    with pytest.raises(SystemExit) as e:
        entrance.main(["prep", "--task", "lits", "--blend", "cosine", "--tta_mirror", "q"])
    assert "--blend" not in str(e.value) and "--tta_mirror" not in str(e.value)


# ---- the weights ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 7, 128])
def test_gauss_weights_follow_the_formula(p):
    wd, wh, ww = hip_ops.blend_weights_host((p, 2 * p, p), "gauss")
    assert wd.dtype == np.float32 and wd.shape == (p,) and wh.shape == (2 * p,) and np.array_equal(wd, ww)
    i = np.arange(p, dtype=np.float64)
    want = np.exp(-0.5 * ((i - (p - 1) / 2) / (p / 8)) ** 2)
    assert np.array_equal(wd, want.astype(np.float32))            # fp64, rounded once
    assert np.array_equal(wd, wd[::-1])                            # symmetric, bit for bit
    assert wd.max() == 1.0 if p % 2 else wd.max() < 1.0             # the peak is a voxel only for odd p
    assert wd.min() >= np.float32(np.exp(-8.0)) and float(wd.min()) ** 3 > 1e-12
    assert float(wd.min()) * float(wh.min()) * float(ww.min()) > 1e-12      # far from the fp32 denormals (1.2e-38)
    if p == 2:
        assert wd.tolist() == [np.float32(np.exp(-2.0))] * 2       # (0 - 0.5) / 0.25 = -2
    if p == 1:
        assert wd.tolist() == [1.0]


def test_uniform_weights_are_ones_and_unknown_kinds_are_refused():
    w = hip_ops.blend_weights_host((3, 1, 5), "uniform")
    assert [v.tolist() for v in w] == [[1.0] * 3, [1.0], [1.0] * 5] and all(v.dtype == np.float32 for v in w)
    assert [len(v) for v in hip_ops.blend_weights_host(4, "gauss")] == [4, 4, 4]
    with pytest.raises(_lib.EffqError):
        hip_ops.blend_weights_host((3, 3, 3), "cosine")
    with pytest.raises(_lib.EffqError):
        hip_ops.blend_weights_host((3, 0, 3), "gauss")


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_header_and_lib_rows_of_the_new_symbols_have_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)

    def ctype(decl):
        return _lib._P if "*" in decl else {"int": _lib._I, "float": _lib._F}[decl.split()[0]]
    for name, nargs in (("effq_window_gather", 17), ("effq_window_put", 10), ("effq_window_stitch", 18)):
        found = re.findall(r"\bint (%s)\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert len(found) == 1, name
        res, got = _lib.SIGNATURES[name]
        assert res == _lib._I and got == [ctype(a) for a in found[0][1].split(",")] and len(got) == nargs, name
        assert hasattr(_lib.load(), name)
    # and no other window symbol: the mirrored gather and the weighted stitch are these, not entry points of their own
    three = {"effq_window_gather", "effq_window_put", "effq_window_stitch"}
    assert set(re.findall(r"\beffq_window_\w+", hdr)) == three == {n for n in _lib.SIGNATURES if "_window_" in n}
    mk = open(os.path.join(ROOT, "efficientq_amd", "csrc", "Makefile")).read()
    assert " window.hip" in mk and "seg_window.h" in mk
    src = open(os.path.join(ROOT, "efficientq_amd", "csrc", "window.hip")).read()
    assert not re.search(r"atomic\w*\s*\(", re.sub(r"//.*", "", src))       # one owner per element: no atomics at all
    assert '#include "seg_window.h"' in src


# ---- the window function and the predict mission on the host ----------------------------------------------------------------
class BlendOps(PredictOps):
    """PredictOps with the weighted stitch in fp64 on the host (ref_blend) and a record of the calls and their
    arguments."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def window_gather(self, vol, patch, overlap, first=0, count=None, flip=0):
        self.calls.append(("gather", first, flip))
        return super().window_gather(vol, patch, overlap, first, count, flip)

    def window_put(self, last, buf_slice, flip=0, accumulate=False):
        self.calls.append(("put", flip, bool(accumulate)))
        super().window_put(last, buf_slice, flip, accumulate)

    def blend_weights(self, patch, kind="uniform"):
        return tuple(torch.from_numpy(w) for w in hip_ops.blend_weights_host(patch, kind))

    def window_stitch(self, win, shape, patch, overlap, weights=None, nflip=1):
        self.calls.append(("stitch", weights is None, nflip))
        if weights is None and nflip == 1:
            return super().window_stitch(win, shape, patch, overlap)
        weights = self.blend_weights(patch) if weights is None else weights
        out, _, _ = ref_blend([win.numpy()], [w.numpy() for w in weights], tuple(shape), patch, overlap)
        return torch.from_numpy((out / nflip).astype(np.float32))


class EdgeNet(torch.nn.Module):
    """Not flip-equivariant: every voxel also sees its neighbour to the left along w (zero at the border)."""

    def forward(self, x):
        left = torch.nn.functional.pad(x, (1, 0))[..., :-1]
        return torch.cat([x + 2.0 * left, x - left], 1)


def _default_calls_are_one_plain_pass(calls):
    """The record of a default run: every gather un-mirrored, every put a store of mask 0, every stitch without weights
    over one pass - what was gather, copy_, stitch before the window function had one path."""
    assert {c[0] for c in calls} == {"gather", "put", "stitch"}
    assert all(c[2] == 0 for c in calls if c[0] == "gather")
    assert all(c[1:] == (0, False) for c in calls if c[0] == "put")
    assert all(c[1:] == (True, 1) for c in calls if c[0] == "stitch")


def test_window_function_runs_todays_statements_by_default_and_the_passes_otherwise():
    g = torch.Generator().manual_seed(3)
    vol = torch.randn(2, 1, 9, 8, 11, generator=g)
    p, o = (4, 4, 6), (1, 2, 3)
    ops = BlendOps()
    base, nwin, _ = E.stitched_window_logits(ops, [EdgeNet()], vol, p, o, 5)
    _default_calls_are_one_plain_pass(ops.calls)
    assert nwin == 3 * 3 * 3
    want = E.sliding_window_forward(EdgeNet(), vol, p, o)[-1]
    assert torch.equal(base[0], want)
    # every pass of every batch: mirrored gather, forward, put - the first stored, the others added
    ops = BlendOps()
    flips = (0, 2, 4, 6)
    got, nwin, _ = E.stitched_window_logits(ops, [EdgeNet(), EdgeNet()], vol, p, o, 5, "gauss", flips)
    assert {c[0] for c in ops.calls} == {"gather", "put", "stitch"}
    batches = [0, 5, 10, 15, 20, 25]
    assert [c[1:] for c in ops.calls if c[0] == "gather"] == [(b, m) for b in batches for m in flips]
    assert [c[1:] for c in ops.calls if c[0] == "put"] == [(m, m != 0) for b in batches for m in flips for _ in range(2)]
    assert [c for c in ops.calls if c[0] == "stitch"] == [("stitch", False, 4)] * 2           # with weights, 4 passes
    assert torch.equal(got[0], got[1])
    # against the restatement of the whole pipeline in fp64
    net64, passes = EdgeNet().double(), []
    pats = E.image_to_patch3d(vol.double(), p, o)
    for m in flips:
        dims = [2 + b for b in range(3) if m >> b & 1]
        outs = [net64(torch.flip(pt, dims) if dims else pt) for pt in pats]
        outs = [torch.flip(v, dims) if dims else v for v in outs]
        passes.append(torch.cat([v.permute(0, 2, 3, 4, 1) for v in outs]).numpy())
    ref, mag, cover = ref_blend(passes, hip_ops.blend_weights_host(p, "gauss"), (2, 2, 9, 8, 11), p, o)
    err = np.abs(got[0].numpy() - ref)
    assert (err <= blend_bound(mag, cover, len(flips)) + 8 * 2.0 ** -24 * mag).all()      # + the fp32 forward and puts
    assert np.abs(ref - base[0].numpy()).max() > 0.05           # the passes and the weights changed the result
    # uniform blending with mirror passes: no weights reach the stitch, the passes do
    ops = BlendOps()
    uni, _, _ = E.stitched_window_logits(ops, [EdgeNet()], vol, p, o, 5, "uniform", (0, 4))
    assert [c for c in ops.calls if c[0] == "stitch"] == [("stitch", True, 2)]
    assert [c[1:] for c in ops.calls if c[0] == "put"] == [(m, m != 0) for b in batches for m in (0, 4)]
    ref, mag, cover = ref_blend(passes[:1] + passes[2:3], hip_ops.blend_weights_host(p, "uniform"), (2, 2, 9, 8, 11), p, o)
    assert (np.abs(uni[0].numpy() - ref) <= blend_bound(mag, cover, 2) + 8 * 2.0 ** -24 * mag).all()
    for bad in (dict(blend="cosine"), dict(flips=()), dict(flips=(4, 0)), dict(flips=(0, 9))):
        with pytest.raises(ValueError):
            E.stitched_window_logits(BlendOps(), [EdgeNet()], vol, p, o, 5, **bad)


def _run_predict(tmp_path, name, *extra, **over):
    root, out = str(tmp_path), str(tmp_path / name)
    lst = os.path.join(root, "cases.csv")
    if not os.path.exists(lst):
        lst, _ = write_cases(root, ["a", "b"], [1, 2])
    ops = BlendOps()
    rows = predict.run(predict_args(*extra, src_list=lst, out_dir=out, patch_size="8,8,8", prep_mask="nonzero", **over),
                       ops=ops, model=PointNet(), window_batch=3)
    return rows, out, ops


def test_predict_csv_is_unchanged_by_default_and_records_the_switches_otherwise(tmp_path, capsys):
    rows, out, ops = _run_predict(tmp_path, "plain")
    said = capsys.readouterr().out
    assert "passes" not in said and "blend" not in said
    assert written(out) == ["a.nii.gz", "b.nii.gz", "predict.csv"]
    with open(os.path.join(out, predict.PREDICT_CSV), newline="") as f:
        table = list(csv.reader(f))
    assert table[0] == predict.CSV_HEADER and "blend" not in table[0] and len(table) == 3
    assert predict.CSV_HEADER[-1] == "volume_ml" and len(predict.CSV_HEADER) == 15
    _default_calls_are_one_plain_pass(ops.calls)
    assert "blend" not in rows[0] and "tta_mirror" not in rows[0]

    rows2, out2, ops2 = _run_predict(tmp_path, "tta", "--blend", "gauss", "--tta_mirror", "hw")
    said = capsys.readouterr().out
    assert "windows x 4 passes, blend gauss" in said
    table2 = list(csv.DictReader(open(os.path.join(out2, predict.PREDICT_CSV))))
    assert list(table2[0]) == predict.CSV_HEADER + ["blend", "tta_mirror"]
    assert [(r["blend"], r["tta_mirror"]) for r in table2] == [("gauss", "hw")] * 2
    assert {c[0] for c in ops2.calls} == {"gather", "put", "stitch"}
    assert {c[2] for c in ops2.calls if c[0] == "gather"} == {0, 2, 4, 6}
    assert {c[1:] for c in ops2.calls if c[0] == "stitch"} == {(False, 4)}
    # every earlier column holds what it held (PointNet works voxel by voxel: the maps agree as well)
    for r, r2 in zip(rows, rows2):
        assert all(r[k] == r2[k] for k in predict.CSV_HEADER)

    # one switch alone: both columns, the other at its default
    _, out3, _ = _run_predict(tmp_path, "w", tta_mirror="w")
    t3 = list(csv.DictReader(open(os.path.join(out3, predict.PREDICT_CSV))))
    assert (t3[0]["blend"], t3[0]["tta_mirror"]) == ("uniform", "w")
    _, out4, ops4 = _run_predict(tmp_path, "g", blend="gauss")
    t4 = list(csv.DictReader(open(os.path.join(out4, predict.PREDICT_CSV))))
    assert (t4[0]["blend"], t4[0]["tta_mirror"]) == ("gauss", "none")
    assert {c[2] for c in ops4.calls if c[0] == "gather"} == {0}
    assert {c[1:] for c in ops4.calls if c[0] == "stitch"} == {(False, 1)}


def test_predict_refuses_the_switches_by_name_and_leaves_out_dir_empty(tmp_path):
    for over, named in ((dict(tta_mirror="x"), ["--tta_mirror", "'x'"]), (dict(tta_mirror="dd"), ["--tta_mirror", "'dd'"]),
                        (dict(tta_mirror=""), ["--tta_mirror"]), (dict(blend="cosine"), ["--blend", "cosine"])):
        with pytest.raises(SystemExit) as e:
            _run_predict(tmp_path, "refused", **over)
        assert all(n in str(e.value) for n in named), str(e.value)
        assert not os.path.exists(tmp_path / "refused")
