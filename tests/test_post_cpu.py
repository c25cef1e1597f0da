"""--post, host side (no GPU): the rule parser and what it refuses, the C-ABI rows of effq_label_clean and
effq_label_tallies and their argument checks (which run before anything is launched), the numpy restatement on hand-made
cases, and the predict mission and the validation driven through stand-ins for the device ops."""
import csv
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, config as Cf, entrance, evaluate as E, nifti, predict
from tests import cpu_backend, label_clean_ref as R
from tests.test_predict_cpu import PointNet, predict_args, ref_merge, write_cases
from tests.test_prep_cpu import written
from tests.test_window_blend_cpu import BlendOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the parser -------------------------------------------------------------------------------------------------------
def _parse(*argv):
    return Cf.build_parser().parse_args(["ptq"] + list(argv))


def test_rules_parse_in_order_with_their_defaults():
    assert Cf.post_rules(_parse()) == ([], 26)
    rules, conn = Cf.post_rules(_parse("--post", "1,2:largest", "--post", "4:min500>1", "--post", "2:min10>1"))
    assert conn == 26 and rules == [((1, 2), "largest", 0, 0), ((4,), "min", 500, 1), ((2,), "min", 10, 1)]
    assert rules[0].labels == (1, 2) and rules[1].op == "min" and rules[1].n == 500 and rules[1].to == 1
    assert Cf.post_rules(_parse("--post", "7:largest>255", "--post_conn", "6")) == ([((7,), "largest", 0, 255)], 6)
    assert Cf.post_rules(_parse("--post", "3:min1", "--post_conn", "26"))[1] == 26
    assert Cf.make_args(Cf.TINY_NET, 4, 4).post is None and Cf.post_rules(Cf.make_args(Cf.TINY_NET, 4, 4)) == ([], 26)
    assert Cf.POST_MAX_RULES == _lib.LABEL_CLEAN_MAX_RULES == 8


@pytest.mark.parametrize("argv, named", [
    (["--post", "1:biggest"], ["--post", "'1:biggest'", "unknown op", "largest"]),
    (["--post", "1:min"], ["--post", "unknown op", "minN"]),
    (["--post", "1:min0"], ["--post", "'1:min0'", "N", "1 or more"]),
    (["--post", "1:min-4"], ["--post", "N", "1 or more"]),
    (["--post", "0:largest"], ["--post", "label '0'", "1 to 255"]),
    (["--post", "1,256:largest"], ["--post", "label '256'", "1 to 255"]),
    (["--post", "x:largest"], ["--post", "label 'x'", "1 to 255"]),
    (["--post", "1,2:largest>2"], ["--post", "TO 2", "LABELS"]),
    (["--post", "1:min5>256"], ["--post", "TO '256'", "0 to 255"]),
    (["--post", ":largest"], ["--post", "empty LABELS"]),
    (["--post", "largest"], ["--post", "'largest'", "LABELS:OP"]),
    (["--post", "1:largest"] * 9, ["--post", "9 rules", "at most 8"]),
    (["--post_conn", "6"], ["--post_conn", "no --post"]),
    (["--post", "1:largest", "--post_conn", "18"], ["--post_conn", "'18'", "6, 26"]),
])
def test_what_is_not_understood_is_refused_by_name(argv, named):
    with pytest.raises(SystemExit) as e:
        Cf.post_rules(_parse(*argv))
    assert all(n in str(e.value) for n in named), str(e.value)


def test_yaml_list_form_and_the_round_trip_of_the_csv_string(tmp_path):
    cfg = tmp_path / "p.yaml"
    cfg.write_text("post:\n  - '1,2:largest'\n  - '4:min500>1'\npost_conn: 6\n")
    a = Cf.merge_config(str(cfg), _parse("--post", "9:largest"))          # YAML beats the command line
    rules, conn = Cf.post_rules(a)
    assert rules == [((1, 2), "largest", 0, 0), ((4,), "min", 500, 1)] and conn == 6
    cfg.write_text("post: '2:min10>1'\n")                                   # one rule as a scalar
    assert Cf.post_rules(Cf.merge_config(str(cfg), _parse())) == ([((2,), "min", 10, 1)], 26)
    cfg.write_text("post: ['1:min0']\n")
    with pytest.raises(SystemExit) as e:
        Cf.post_rules(Cf.merge_config(str(cfg), _parse()))
    assert "'1:min0'" in str(e.value)
    said = Cf.post_text(rules, conn)
    assert said == "1,2:largest 4:min500>1 conn6" and Cf.parse_post_text(said) == (rules, conn)
    assert Cf.post_text(rules) == "1,2:largest 4:min500>1" and Cf.parse_post_text(Cf.post_text(rules)) == (rules, 26)
    assert Cf.post_rule_text(Cf.parse_post_rule(" 1 , 2 : largest > 0 ")) == "1,2:largest"


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_and_lib_have_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return _lib._P
        if decl.startswith("long long"):
            return _lib._LL
        return {"int": _lib._I, "size_t": _lib._SZ}[decl.split()[0]]
    lib = _lib.load()
    for name, res, nargs in (("effq_label_clean", "int", 13), ("effq_label_clean_ws_bytes", "size_t", 3),
                             ("effq_label_tallies", "int", 10), ("effq_label_tallies_ws_bytes", "size_t", 0)):
        found = re.findall(rf"\b{res} ({name})\s*\((.*?)\)\s*;", code, flags=re.S)
        assert len(found) == 1, name
        args = [a for a in found[0][1].split(",") if a.strip() not in ("", "void")]
        got_res, got = _lib.SIGNATURES[name]
        assert got_res == (_lib._I if res == "int" else _lib._SZ) and got == [ctype(a) for a in args], name
        assert len(got) == nargs and hasattr(lib, name)
    for macro, value in (("EFFQ_LABEL_CLEAN_MAX_RULES", 8), ("EFFQ_LABEL_CLEAN_LARGEST", 0), ("EFFQ_LABEL_CLEAN_MIN", 1)):
        assert re.search(rf"#define {macro} {value}\b", code)
    assert _lib.LABEL_CLEAN_OPS == {"largest": 0, "min": 1}
    assert "equal inputs give equal bits" in hdr[hdr.index("cleaning a predicted label map"):hdr.index("effq_label_clean_ws_bytes(int")]


def test_argument_checks_run_before_anything_is_launched():
    """No device is needed to be refused: the pointers below are never followed."""
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    sets = (C.c_uint8 * 512)()
    sets[1] = sets[256 + 2] = 1

    def clean(R_=2, words=(0, 0, 0, 1, 3, 0), conn=26, dims=(4, 5, 6), s=sets, ws_bytes=1 << 20, **null):
        p = dict(inp=fake, out=fake, stats=fake, ws=fake, sets=s, rules=(C.c_longlong * 6)(*words))
        p.update(null)
        return lib.effq_label_clean(p["inp"], *dims, conn, R_, p["sets"], p["rules"], p["out"], p["stats"], p["ws"],
                                    ws_bytes, None)
    ARG, WS = 1, 3
    assert (_lib._ERR_NAMES[ARG], _lib._ERR_NAMES[WS]) == ("EFFQ_ERR_ARG", "EFFQ_ERR_WORKSPACE")
    for name in ("inp", "out", "stats", "ws", "sets", "rules"):
        assert clean(**{name: None}) == ARG, name
    assert clean(R_=0) == ARG and clean(R_=9) == ARG
    assert clean(words=(2, 0, 0, 1, 3, 0)) == ARG and clean(words=(0, 0, 0, 1, 0, 0)) == ARG
    assert clean(words=(0, 0, 256, 1, 3, 0)) == ARG and clean(words=(0, 0, -1, 1, 3, 0)) == ARG
    assert clean(words=(0, 0, 1, 1, 3, 0)) == ARG and clean(words=(0, 0, 0, 1, 3, 2)) == ARG
    zero = (C.c_uint8 * 512)()
    zero[0] = zero[1] = 1
    assert clean(s=zero) == ARG
    assert clean(conn=18) == ARG and clean(dims=(0, 5, 6)) == ARG and clean(dims=(2048, 1024, 1024)) == ARG
    assert "argument check failed" in lib.effq_last_error().decode()
    need = lib.effq_label_clean_ws_bytes(4, 5, 6)
    assert need >= 9 * 120 and lib.effq_label_clean_ws_bytes(0, 5, 6) == 0
    assert lib.effq_label_clean_ws_bytes(2048, 1024, 1024) == 0
    # 4 B of label, 4 B of size and 1 B of mask per voxel, each rounded up to 16 B, and the counters
    big = lib.effq_label_clean_ws_bytes(155, 240, 240)
    assert big == 512 * 2 * 4 + 2 * 4 * 155 * 240 * 240 + 155 * 240 * 240 + 64
    assert clean(ws_bytes=need - 1) == WS and "needs" in lib.effq_last_error().decode()
    lut = (C.c_uint16 * 256)()
    tally = lambda C_=3, S=20, **null: lib.effq_label_tallies(
        null.get("pred", fake), null.get("truth", fake), 0, C_, S, null.get("lut", lut), null.get("counts", fake),
        null.get("ws", fake), null.get("ws_bytes", 1 << 20), None)
    for name in ("pred", "truth", "lut", "counts", "ws"):
        assert tally(**{name: None}) == ARG, name
    assert tally(C_=0) == ARG and tally(C_=9) == ARG and tally(S=0) == ARG
    assert tally(ws_bytes=lib.effq_label_tallies_ws_bytes() - 1) == WS
    assert 0 < lib.effq_label_tallies_ws_bytes() <= _lib.SEG_TALLIES_WS_BYTES


# ---- the restatement on hand-made cases -----------------------------------------------------------------------------------
def test_restatement_on_cases_with_known_answers():
    a = np.zeros((3, 4, 6), dtype=np.uint8)
    a[0, 0, 0:3] = 1                       # 3 voxels
    a[1, 1, 3] = 2                         # touches the run by a corner only: (0, 0, 2) - (1, 1, 3)
    a[2, 3, 4:6] = 1                       # 2 voxels
    names = R.first_voxels(a > 0, 26)
    assert sorted(set(names[names >= 0].tolist())) == [0, 2 * 24 + 3 * 6 + 4] and names[1, 1, 3] == 0
    assert len(R.component_sizes(R.first_voxels(a > 0, 6))[0]) == 3
    out, st = R.clean(a, [((1, 2), "largest", 0, 0)], 26)
    assert st.tolist() == [[2, 2]] and out[2].sum() == 0 and out[:2].tolist() == a[:2].tolist()
    out, st = R.clean(a, [((1, 2), "largest", 0, 9)], 6)
    assert st.tolist() == [[3, 3]] and out[1, 1, 3] == 9 and (out[2, 3, 4:6] == 9).all() and (out[0, 0, :3] == 1).all()
    out, st = R.clean(a, [((1,), "min", 3, 2), ((2,), "largest", 0, 0)], 26)       # the pair becomes 2 and then loses
    assert st.tolist() == [[2, 2], [2, 1]] and out[1, 1, 3] == 0 and (out[2, 3, 4:6] == 2).all()
    out, st = R.clean(a, [((1,), "min", 2, 0)], 26)                                 # size == N stays
    assert st.tolist() == [[2, 0]] and np.array_equal(out, a)
    # equal sizes: the least first voxel stays
    b = np.zeros((2, 2, 8), dtype=np.uint8)
    b[0, 0, 5:7] = 3
    b[1, 1, 0:2] = 3
    out, st = R.clean(b, [((3,), "largest", 0, 0)], 26)
    assert (out[0, 0, 5:7] == 3).all() and out.sum() == 6 and st.tolist() == [[2, 2]]
    # tallies: the map form and the planes form, and the validation's tables
    lut = R.class_lut("brats", 3)
    assert lut == E.post_class_lut("brats", 3) and R.class_lut("argmax", 3) == E.post_class_lut("argmax", 3)
    pred = np.array([0, 1, 2, 4, 4], dtype=np.uint8)
    truth = np.array([1, 1, 0, 2, 4], dtype=np.uint8)
    want = [[3, 1, 1, 0], [2, 1, 1, 1], [1, 1, 0, 3]]
    assert R.tallies(pred, truth, lut, 3).tolist() == want
    planes = np.stack([(np.array(lut)[truth] >> c) & 1 for c in range(3)]).astype(np.uint8)
    assert R.tallies(pred, planes * 5, lut, 3).tolist() == want


# ---- stand-ins for the device ---------------------------------------------------------------------------------------------
class PostOps(cpu_backend.OracleOps, BlendOps):
    """The CPU backend with the window ops of the predict tests, the decisions in torch, and label_clean and
    label_tallies through the numpy restatement; for the orchestration tests only."""

    def __init__(self):
        BlendOps.__init__(self)
        self.device = torch.device("cpu")
        self.cleaned = []

    @staticmethod
    def _bits(logits, fuse):
        return ref_merge(logits.numpy() >= 0.0, fuse)

    def seg_labels(self, logits, rule, fuse=None, dtype=torch.uint8):
        if rule == "argmax":
            return logits.argmax(1).to(dtype)
        assert rule == "brats"
        bits = np.stack([self._bits(x, fuse) for x in logits])
        lab = np.zeros(bits[:, 0].shape, dtype=np.uint8)
        lab[bits[:, 0]] = 1
        lab[bits[:, 0] & ~bits[:, 1]] = 2
        lab[bits[:, 2]] = 4
        return torch.from_numpy(lab).to(dtype)

    def seg_tallies(self, logits, label, task, fuse=None):
        Cc = logits.shape[0]
        if task == "lits":
            p = logits.argmax(0).numpy()
            pred = np.stack([p == c for c in range(Cc)])
            gt = np.stack([label.numpy() == c for c in range(Cc)])
        else:
            pred, gt = self._bits(logits, fuse), label.numpy() != 0
        return torch.tensor([[(p & g).sum(), (p & ~g).sum(), (~p & g).sum(), (~p & ~g).sum()] for p, g in zip(pred, gt)])

    def label_clean(self, label_map, rules, connectivity=26, out=None):
        self.cleaned.append((tuple(label_map.shape), list(rules), connectivity, out is label_map))
        got, stats = R.clean(label_map.numpy(), rules, connectivity)
        if out is None:
            out = torch.empty_like(label_map)
        out.copy_(torch.from_numpy(got))
        return out, torch.from_numpy(stats)

    def label_tallies(self, pred, truth, lut, C_):
        return torch.from_numpy(R.tallies(pred.numpy(), truth.numpy(), lut, C_))


class SpeckNet(PointNet):
    """PointNet with a parameter, so that validate_seg finds its device."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


# ---- predict --------------------------------------------------------------------------------------------------------------
def _predict(tmp_path, name, *extra, **over):
    root, out = str(tmp_path), str(tmp_path / name)
    lst = os.path.join(root, "cases.csv")
    if not os.path.exists(lst):
        lst, _ = write_cases(root, ["a", "b"], [1, 2])
    ops = PostOps()
    rows = predict.run(predict_args(*extra, src_list=lst, out_dir=out, patch_size="8,8,8", prep_mask="nonzero", **over),
                       ops=ops, model=PointNet(), window_batch=3)
    with open(os.path.join(out, predict.PREDICT_CSV), newline="") as f:
        return rows, out, ops, list(csv.reader(f))


def test_predict_cleans_the_map_on_the_source_grid_and_adds_its_two_columns_last(tmp_path, capsys):
    _, plain, ops0, t0 = _predict(tmp_path, "plain")
    assert t0[0] == predict.CSV_HEADER and ops0.cleaned == [] and "post" not in capsys.readouterr().out
    post = ["--post", "1:largest", "--post", "2:min4>1"]
    # faces only: PointNet decides voxel by voxel, so the classes of its maps fall into many small components
    rows, out, ops, t1 = _predict(tmp_path, "post", "--post_conn", "6", *post)
    said = capsys.readouterr().out
    assert t1[0] == predict.CSV_HEADER + ["post", "post_changed"] and predict.CSV_POST_COLUMNS == ["post", "post_changed"]
    assert written(out) == ["a.nii.gz", "b.nii.gz", "predict.csv"]
    rules = [((1,), "largest", 0, 0), ((2,), "min", 4, 1)]
    assert ops.cleaned == [((20, 24, 28), rules, 6, True)] * 2             # on the scans' own grid, in place
    for r0, r1, row in zip(t0[1:], t1[1:], rows):
        sn = r1[0]
        before, _ = nifti.read_nifti(os.path.join(plain, f"{sn}.nii.gz"))
        after, _ = nifti.read_nifti(os.path.join(out, f"{sn}.nii.gz"))
        want, stats = R.clean(before, rules, 6)
        assert np.array_equal(after, want) and after.dtype == np.uint8
        assert r1[-2] == "1:largest 2:min4>1 conn6" and Cf.parse_post_text(r1[-2]) == (rules, 6)
        changed = [int(v) for v in r1[-1].split()]
        assert changed == stats[:, 1].tolist() and min(changed) > 0
        assert f"post 1:largest 2:min4>1 conn6: {r1[-1]} voxels relabelled" in said
        # every column before labels holds what it held; labels, voxels and volume_ml are the cleaned map's
        k = predict.CSV_HEADER.index("labels")
        assert r0[:k] == r1[:k] and r0[k:15] != r1[k:15] and row["post_changed"] == r1[-1]
        count = np.bincount(after.ravel())
        assert [int(v) for v in r1[k].split()] == [v for v in range(len(count)) if count[v]]
        assert [int(v) for v in r1[k + 1].split()] == [int(n) for n in count if n]
    # after blend and tta_mirror when those are present; the default neighbourhood is not written out
    _, out2, ops2, t2 = _predict(tmp_path, "both", "--blend", "gauss", *post)
    assert t2[0] == predict.CSV_HEADER + ["blend", "tta_mirror", "post", "post_changed"]
    assert t2[1][-2] == "1:largest 2:min4>1" and ops2.cleaned[0][2] == 26
    before, _ = nifti.read_nifti(os.path.join(plain, "a.nii.gz"))          # voxel by voxel: the blend leaves the map
    want, stats = R.clean(before, rules, 26)
    assert np.array_equal(nifti.read_nifti(os.path.join(out2, "a.nii.gz"))[0], want)
    assert [int(v) for v in t2[1][-1].split()] == stats[:, 1].tolist()
    _, _, _, t3 = _predict(tmp_path, "blend", "--blend", "gauss")
    assert t3[0] == predict.CSV_HEADER + ["blend", "tta_mirror"]
    # without --post the file is byte for byte the parent's: the same header, and the code path is not entered
    again = _predict(tmp_path, "again")
    assert again[2].cleaned == []
    assert open(os.path.join(plain, "predict.csv"), "rb").read() == open(os.path.join(again[1], "predict.csv"), "rb").read()


def test_predict_refuses_before_out_dir_exists(tmp_path):
    root, out = str(tmp_path), str(tmp_path / "seg")
    lst, _ = write_cases(root, ["a"], [1])
    for over, named in ((dict(post=["1:biggest"]), ["--post", "unknown op"]),
                        (dict(post_conn="6"), ["--post_conn", "no --post"]),
                        (dict(post=["1:largest"], multi_label="lits"), ["--multi_label lits", "plane"])):
        with pytest.raises(SystemExit) as e:
            predict.run(predict_args(src_list=lst, out_dir=out, patch_size="8,8,8", **over), ops=PostOps(),
                        model=PointNet(), window_batch=2)
        assert all(n in str(e.value) for n in named), str(e.value)
        assert not os.path.exists(out)
    # predict scores nothing: the merged map of un-nested brats planes is cleaned like any other, so the next thing
    # that stops this run is its list
    with pytest.raises(FileNotFoundError) as e:
        predict.run(predict_args(src_list=os.path.join(root, "none.csv"), out_dir=out, patch_size="8,8,8",
                                 post=["4:min5>1"], multi_label="brats"), ops=PostOps(), model=PointNet(), window_batch=2)
    assert "none.csv" in str(e.value) and "--merge_type" not in str(e.value) and not os.path.exists(out)


# ---- the validation -----------------------------------------------------------------------------------------------------------
def _lits_loader(n=2, shape=(10, 12, 14)):
    g = torch.Generator().manual_seed(4)
    return [(torch.randn(1, 1, *shape, generator=g), torch.randint(0, 3, (1,) + shape, generator=g)) for _ in range(n)]


class BratsNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return torch.cat([x[:, :1] + 0.6, x[:, 1:2] + x[:, :1], x[:, 2:3] - 0.5], 1)


def test_validate_seg_scores_the_cleaned_map_and_leaves_the_rest(monkeypatch):
    from efficientq_amd import hip_ops
    ops = PostOps()
    monkeypatch.setattr(hip_ops, "get_ops", lambda dev: ops)
    rules = [((1, 2), "largest", 0, 0), ((2,), "min", 3, 1)]
    loader = _lits_loader()
    kw = dict(task="lits", patch_size=(8, 8, 8), overlap=(2, 2, 2), window_batch=4, names=["s1", "s2"])
    base = E.validate_seg(SpeckNet(), loader, **kw)
    res = E.validate_seg(SpeckNet(), loader, post=rules, post_conn=6, **kw)
    assert [c[1:3] for c in ops.cleaned] == [(rules, 6)] * 2 and not any(c[3] for c in ops.cleaned)
    for r0, r, (img, lab) in zip(base, res, loader):
        assert "post" not in r0 and sorted(r) == sorted(list(r0) + ["post"])
        assert all(torch.equal(r0[k], r[k]) for k in ("counts",) + E.METRICS)
        logits, _, _ = E.stitched_window_logits(ops, [SpeckNet()], img, (8, 8, 8), (2, 2, 2), 4)
        pmap = logits[0][0].argmax(0).numpy().astype(np.uint8)
        want, stats = R.clean(pmap, rules, 6)
        counts = R.tallies(want, lab[0].numpy().astype(np.uint8), R.class_lut("argmax", 3), 3)
        q = r["post"]
        assert sorted(q) == sorted(("counts", "changed") + E.METRICS)
        assert q["counts"].tolist() == counts.tolist() and q["changed"] == stats[:, 1].tolist() and sum(q["changed"]) > 0
        assert all(torch.equal(q[m], E.metrics_from_counts(torch.from_numpy(counts))[m]) for m in E.METRICS)
        assert q["counts"].tolist() != r["counts"].tolist()
    # brats: the loader's three planes are the truth, the map's values are read back through the table
    g = torch.Generator().manual_seed(9)
    bl = [(torch.randn(1, 4, 9, 10, 11, generator=g), (torch.rand(1, 3, 9, 10, 11, generator=g) < 0.4).to(torch.uint8))]
    brats = dict(task="brats", patch_size=(8, 8, 8), overlap=(2, 2, 2), window_batch=4, multi_label="brats")
    for fuse in ("agg", "con"):
        r = E.validate_seg(BratsNet(), bl, fuse=fuse, post=[((4,), "min", 3, 1)], **brats)[0]
        logits, _, _ = E.stitched_window_logits(ops, [BratsNet()], bl[0][0], (8, 8, 8), (2, 2, 2), 4)
        pmap = ops.seg_labels(logits[0], "brats", fuse)[0].numpy()
        assert sorted(np.unique(pmap).tolist()) == [0, 1, 2, 4]
        # un-cleaned, the table gives the tallies of the logits themselves: the planes are read back exactly
        lut = R.class_lut("brats", 3)
        assert R.tallies(pmap, bl[0][1][0].numpy(), lut, 3).tolist() == r["counts"].tolist()
        want, stats = R.clean(pmap, [((4,), "min", 3, 1)], 26)
        assert r["post"]["counts"].tolist() == R.tallies(want, bl[0][1][0].numpy(), lut, 3).tolist()
        assert r["post"]["changed"] == [int(stats[0, 1])] and stats[0, 1] > 0
    for bad, named in ((dict(fuse=None), "--merge_type"), (dict(fuse="agg", multi_label="lits"), "--multi_label lits")):
        with pytest.raises(RuntimeError) as e:
            E.validate_seg(BratsNet(), bl, post=[((4,), "min", 3, 1)], **dict(brats, **bad))
        assert named in str(e.value)


def test_metrics_post_csv_layout_and_the_tester_writes_it_beside_metrics_csv(tmp_path, monkeypatch, capsys):
    from efficientq_amd import hip_ops
    ops = PostOps()
    monkeypatch.setattr(hip_ops, "get_ops", lambda dev: ops)
    rules = [((1, 2), "largest", 0, 0), ((2,), "min", 3, 1)]
    cube = types.SimpleNamespace(valloader=_lits_loader(), val_sn=["s1", "s2"], patch_size=(8, 8, 8), overlap=(2, 2, 2),
                                 multilabel_fusetype=None, multi_label=None, labelled=True, geometry=None, spacing=None)
    plain, post = str(tmp_path / "plain"), str(tmp_path / "post")
    whole = E.validate_seg                  # the tester leaves the window batch to the device's memory: fixed here
    monkeypatch.setattr(E, "validate_seg", lambda *a, **k: whole(*a, window_batch=4, **k))
    entrance._ValidationTester(SpeckNet(), plain, cube, "lits").test_as_is("ptq")
    capsys.readouterr()
    entrance._ValidationTester(SpeckNet(), post, cube, "lits", post=rules, post_conn=26).test_as_is("ptq")
    said = capsys.readouterr().out
    assert "--post 1,2:largest 2:min3>1" in said and "before -> after" in said
    assert written(os.path.join(plain, "ptq")) == ["metrics.csv"]
    assert written(os.path.join(post, "ptq")) == ["metrics.csv", "metrics_post.csv"]
    same = lambda f: open(os.path.join(plain, "ptq", f), "rb").read() == open(os.path.join(post, "ptq", f), "rb").read()
    assert same("metrics.csv")
    with open(os.path.join(post, "ptq", "metrics_post.csv"), newline="") as f:
        table = list(csv.reader(f))
    assert table[0] == ["subject", "class", "dsc", "sens", "spec", "acc", "tp", "fp", "fn", "tn", "changed_0", "changed_1"]
    assert [(r[0], r[1]) for r in table[1:]] == [(s, str(c)) for s in ("s1", "s2") for c in range(3)]
    res = whole(SpeckNet(), cube.valloader, "lits", (8, 8, 8), (2, 2, 2), names=cube.val_sn, post=rules, window_batch=4)
    for row in table[1:]:
        q = next(r for r in res if r["name"] == row[0])["post"]
        c = int(row[1])
        assert [int(v) for v in row[6:10]] == q["counts"][c].tolist() and [int(v) for v in row[10:]] == q["changed"]
        assert row[2:6] == ["%.7g" % float(q[m][c]) for m in E.METRICS]
        assert sum(int(v) for v in row[6:10]) == 10 * 12 * 14


@pytest.mark.parametrize("argv, named", [
    (["ptq", "--task", "lits", "--multi_label", "lits", "--post", "1:largest"], ["--post", "--multi_label lits", "plane"]),
    (["ptq", "--task", "brats", "--multi_label", "brats", "--post", "4:min500>1"],
     ["--post", "--multi_label brats", "--merge_type"]),
    (["ptq", "--task", "lits", "--unlabelled", "--vs_fp", "--post", "1:largest"], ["--post", "--unlabelled"]),
    (["ptq", "--task", "lits", "--synthetic", "--post", "1:largest"], ["--post", "--synthetic", "labels"]),
    (["ptq", "--task", "lits", "--synthetic", "--vs_fp", "--post", "1:largest"], ["--post", "--synthetic"]),
    (["prep", "--task", "lits", "--post", "1:largest"], ["--post", "prep"]),
    (["ptq", "--task", "lits", "--post", "1:smallest"], ["--post", "unknown op"]),
    (["ptq", "--task", "lits", "--post_conn", "6"], ["--post_conn", "no --post"]),
])
def test_the_missions_refuse_by_name_before_anything_is_created(tmp_path, argv, named):
    snap, data = str(tmp_path / "snap"), str(tmp_path / "data")
    with pytest.raises(SystemExit) as e:
        entrance.main(argv + ["--snap_dir", snap, "--data_dir", data, "--split_dir", str(tmp_path / "split"),
                              "--src_list", str(tmp_path / "none.csv"), "--qlvl_w", "4", "--qlvl_a", "4"])
    assert all(n in str(e.value) for n in named), str(e.value)
    assert os.listdir(str(tmp_path)) == []
    # with --merge_type the brats rule goes through the check
    if "brats" in argv:
        a = Cf.build_parser().parse_args(argv + ["--merge_type", "agg"])
        assert entrance.check_post(a) == ([((4,), "min", 500, 1)], 26)
