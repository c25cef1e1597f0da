"""--post fill / closeR / openR, host side (no GPU): the rule language and what it refuses, the C-ABI rows of
effq_label_post and its argument checks (which run before anything is launched), and the numpy / scipy restatement on
hand-made cases whose answers are written out."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from efficientq_amd import _lib, config as Cf, entrance
from tests import label_morph_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the parser -------------------------------------------------------------------------------------------------------
def _parse(*argv):
    return Cf.build_parser().parse_args(["ptq"] + list(argv))


def test_the_new_rules_parse_with_their_defaults():
    one = Cf.parse_post_rule
    assert one("1,2:fill") == ((1, 2), "fill", 0, 1) and one("2,1:fill") == ((2, 1), "fill", 0, 2)
    assert one("1,2:fill>2") == ((1, 2), "fill", 0, 2)
    assert one("1:close2") == ((1,), "close", 2, 1) and one("1,2:close32>2") == ((1, 2), "close", 32, 2)
    assert one("2:open3") == ((2,), "open", 3, 0) and one("2:open1>1") == ((2,), "open", 1, 1)
    assert one(" 1 , 2 : close 3 > 1 ") == ((1, 2), "close", 3, 1)
    r = one("4:open32>255")
    assert (r.labels, r.op, r.n, r.to) == ((4,), "open", 32, 255)
    rules, conn = Cf.post_rules(_parse("--post", "1,2:largest", "--post", "1,2:fill>1", "--post", "2:min10>1",
                                       "--post", "2:open1>1", "--post_conn", "6"))
    assert conn == 6 and rules == [((1, 2), "largest", 0, 0), ((1, 2), "fill", 0, 1), ((2,), "min", 10, 1),
                                   ((2,), "open", 1, 1)]
    assert Cf.POST_MAX_RADIUS == _lib.LABEL_POST_MAX_RADIUS == 32
    assert "fill" in Cf.build_parser().format_help() and "openR" in Cf.build_parser().format_help()


@pytest.mark.parametrize("rule, named", [
    ("1:close", ["unknown op", "'close'", "largest", "minN", "fill, closeR, openR (R voxels)"]),
    ("1:open", ["unknown op", "'open'", "largest, minN (N voxels), fill, closeR, openR (R voxels)"]),
    ("1:close0", ["R", "1 to 32"]),
    ("1:open33", ["R", "1 to 32"]),
    ("1:close-2", ["R", "1 to 32"]),
    ("1,2:fill>3", ["TO 3", "not one of LABELS"]),
    ("1:close2>0", ["TO 0", "not one of LABELS"]),
    ("1:open2>1", ["TO 1", "is one of LABELS"]),
    ("1:fill2", ["unknown op", "'fill2'"]),
    ("1:biggest", ["unknown op", "largest"]),
    ("1:smallest", ["unknown op", "minN"]),
])
def test_what_is_not_understood_is_refused_by_name(rule, named):
    with pytest.raises(SystemExit) as e:
        Cf.post_rules(_parse("--post", rule))
    said = str(e.value)
    assert "--post" in said and repr(rule) in said and all(n in said for n in named), said


def test_round_trip_of_the_csv_string_the_yaml_list_and_mixed_chains(tmp_path):
    text = ["1,2:largest", "1,2:fill>1", "1,2:close2>1", "2:open1>1", "2:min5>1", "3:open4", "3,1:fill"]
    rules = [Cf.parse_post_rule(t) for t in text]
    assert [Cf.post_rule_text(r) for r in rules] == text[:-1] + ["3,1:fill>3"]        # fill and close always say >TO
    assert Cf.post_rule_text(((1,), "close", 3, 1)) == "1:close3>1" and Cf.post_rule_text(((2,), "open", 3, 0)) == "2:open3"
    for conn in (26, 6):
        said = Cf.post_text(rules, conn)
        assert Cf.parse_post_text(said) == (rules, conn)
    assert Cf.post_text(rules, 6).endswith("3:open4 3,1:fill>3 conn6")
    cfg = tmp_path / "p.yaml"
    cfg.write_text("post:\n  - '1,2:largest'\n  - '1,2:fill>1'\n  - '2:open1>1'\npost_conn: 6\n")
    got = Cf.post_rules(Cf.merge_config(str(cfg), _parse()))
    assert got == ([((1, 2), "largest", 0, 0), ((1, 2), "fill", 0, 1), ((2,), "open", 1, 1)], 6)
    cfg.write_text("post: '1:close2'\n")
    assert Cf.post_rules(Cf.merge_config(str(cfg), _parse())) == ([((1,), "close", 2, 1)], 26)
    cfg.write_text("post: ['1:close0']\n")
    with pytest.raises(SystemExit) as e:
        Cf.post_rules(Cf.merge_config(str(cfg), _parse()))
    assert "'1:close0'" in str(e.value)


@pytest.mark.parametrize("argv, named", [
    (["ptq", "--task", "lits", "--multi_label", "lits", "--post", "1:fill"], ["--post", "--multi_label lits", "plane"]),
    (["ptq", "--task", "brats", "--multi_label", "brats", "--post", "1,2,4:fill>2"],
     ["--post", "--multi_label brats", "--merge_type"]),
    (["ptq", "--task", "lits", "--unlabelled", "--vs_fp", "--post", "1:close2"], ["--post", "--unlabelled"]),
    (["ptq", "--task", "lits", "--synthetic", "--post", "2:open1"], ["--post", "--synthetic"]),
    (["prep", "--task", "lits", "--post", "1:fill"], ["--post", "prep"]),
    (["ptq", "--task", "lits", "--post", "1:open33"], ["--post", "1 to 32"]),
])
def test_the_missions_refuse_the_new_rules_as_they_refuse_the_old(tmp_path, argv, named):
    with pytest.raises(SystemExit) as e:
        entrance.main(argv + ["--snap_dir", str(tmp_path / "snap"), "--data_dir", str(tmp_path / "data"),
                              "--split_dir", str(tmp_path / "split"), "--src_list", str(tmp_path / "none.csv"),
                              "--qlvl_w", "4", "--qlvl_a", "4"])
    assert all(n in str(e.value) for n in named), str(e.value)
    assert os.listdir(str(tmp_path)) == []


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
    for name, res, nargs in (("effq_label_post", "int", 13), ("effq_label_post_ws_bytes", "size_t", 4)):
        found = re.findall(rf"\b{res} ({name})\s*\((.*?)\)\s*;", code, flags=re.S)
        assert len(found) == 1, name
        args = [a for a in found[0][1].split(",") if a.strip() not in ("", "void")]
        got_res, got = _lib.SIGNATURES[name]
        assert got_res == (_lib._I if res == "int" else _lib._SZ) and got == [ctype(a) for a in args], name
        assert len(got) == nargs and hasattr(lib, name)
    assert _lib.SIGNATURES["effq_label_post"] == _lib.SIGNATURES["effq_label_clean"]
    for macro, value in (("EFFQ_LABEL_POST_FILL", 2), ("EFFQ_LABEL_POST_CLOSE", 3), ("EFFQ_LABEL_POST_OPEN", 4),
                         ("EFFQ_LABEL_POST_MAX_RADIUS", 32)):
        assert re.search(rf"#define {macro} {value}\b", code)
    assert _lib.LABEL_POST_OPS == {"fill": 2, "close": 3, "open": 4} and _lib.LABEL_CLEAN_OPS == {"largest": 0, "min": 1}
    doc = hdr[hdr.index("filling holes and closing or opening masks"):hdr.index("effq_label_post_ws_bytes(int")]
    assert "equal inputs give equal bits" in doc and "129 071 568 B" in doc


def test_argument_checks_run_before_anything_is_launched():
    """No device is needed to be refused: the pointers below are never followed."""
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    sets = (C.c_uint8 * 512)()
    sets[1] = sets[256 + 2] = 1                      # rule 0: {1}, rule 1: {2}

    def post(R_=2, words=(2, 0, 1, 4, 3, 0), conn=26, dims=(4, 5, 6), s=sets, ws_bytes=1 << 20, **null):
        p = dict(inp=fake, out=fake, stats=fake, ws=fake, sets=s, rules=(C.c_longlong * 6)(*words))
        p.update(null)
        return lib.effq_label_post(p["inp"], *dims, conn, R_, p["sets"], p["rules"], p["out"], p["stats"], p["ws"],
                                   ws_bytes, None)
    ARG, WS = 1, 3
    assert (_lib._ERR_NAMES[ARG], _lib._ERR_NAMES[WS]) == ("EFFQ_ERR_ARG", "EFFQ_ERR_WORKSPACE")
    for name in ("inp", "out", "stats", "ws", "sets", "rules"):
        assert post(**{name: None}) == ARG, name
    assert "argument check failed" in lib.effq_last_error().decode()
    assert post(R_=0) == ARG and post(R_=9) == ARG
    assert post(words=(5, 0, 1, 4, 3, 0)) == ARG and post(words=(-1, 0, 0, 4, 3, 0)) == ARG          # unknown op
    assert post(words=(3, 0, 1, 4, 3, 0)) == ARG and post(words=(3, 33, 1, 4, 3, 0)) == ARG          # close: radius
    assert post(words=(2, 0, 1, 4, 0, 0)) == ARG and post(words=(2, 0, 1, 4, 33, 0)) == ARG          # open: radius
    assert post(words=(2, 0, 1, 4, -2, 0)) == ARG
    assert post(words=(2, 0, 0, 4, 3, 0)) == ARG and post(words=(2, 0, 2, 4, 3, 0)) == ARG           # fill: TO not in the set
    assert post(words=(3, 2, 3, 4, 3, 0)) == ARG                                                      # close: the same
    assert post(words=(2, 0, 1, 4, 3, 2)) == ARG                                                      # open: TO in the set
    assert post(words=(0, 0, 1, 4, 3, 0)) == ARG and post(words=(1, 5, 1, 4, 3, 0)) == ARG           # largest, min: the same
    assert post(words=(1, 0, 0, 4, 3, 0)) == ARG                                                      # min: N < 1
    assert post(words=(2, 0, 256, 4, 3, 0)) == ARG and post(words=(2, 0, 1, 4, 3, -1)) == ARG
    zero = (C.c_uint8 * 512)()
    zero[0] = zero[1] = zero[256 + 2] = 1
    assert post(s=zero) == ARG
    assert post(conn=18) == ARG and post(dims=(0, 5, 6)) == ARG and post(dims=(2048, 1024, 1024)) == ARG
    # the padded plane must satisfy the distance transform's limits: a line of the h pass, and fewer than 2^31 voxels
    assert post(dims=(2, 16380, 2), ws_bytes=1 << 40) == ARG and post(dims=(1290, 1290, 1290), ws_bytes=1 << 40) == ARG
    assert "argument check failed" in lib.effq_last_error().decode()
    ws = lib.effq_label_post_ws_bytes
    assert ws(0, 5, 6, 0) == 0 and ws(2048, 1024, 1024, 0) == 0 and ws(4, 5, 6, -1) == 0 and ws(4, 5, 6, 33) == 0
    assert ws(2, 16380, 2, 2) == 0 and ws(2, 16380, 2, 0) > 0 and ws(2, 16378, 2, 2) > 0
    assert ws(1290, 1290, 1290, 0) > 0 and ws(1290, 1290, 1290, 1) == 0
    # effq_label_clean's, 16 B, and 1 B of site and 4 B of squared distance per voxel of the padded plane
    clean = lib.effq_label_clean_ws_bytes
    assert ws(4, 5, 6, 0) == clean(4, 5, 6) + 16
    assert ws(4, 5, 6, 3) == clean(4, 5, 6) + 16 + 1328 + 4 * 1320              # 10 x 11 x 12 = 1320 padded voxels
    assert ws(155, 240, 240, 3) == clean(155, 240, 240) + 16 + 9743088 + 4 * 9743076 == 129071568
    need = ws(4, 5, 6, 3)
    assert post(ws_bytes=need - 1) == WS and "needs" in lib.effq_last_error().decode()
    assert post(words=(2, 0, 1, 4, 2, 0), ws_bytes=ws(4, 5, 6, 2) - 1) == WS                  # sized by the largest radius
    assert post(words=(2, 0, 1, 1, 3, 0), ws_bytes=ws(4, 5, 6, 0) - 1) == WS
    # effq_label_clean still knows two ops only
    words = (C.c_longlong * 6)(2, 0, 1, 1, 3, 0)
    assert lib.effq_label_clean(fake, 4, 5, 6, 26, 2, sets, words, fake, fake, fake, 1 << 20, None) == ARG


# ---- the restatement on hand-made cases -----------------------------------------------------------------------------------
def _shell():
    a = np.zeros((9, 9, 9), dtype=np.uint8)
    a[2:7, 2:7, 2:7] = 1
    a[3:6, 3:6, 3:6] = 0
    return a


def test_restatement_fills_the_holes_of_cases_with_known_answers():
    a = _shell()
    for conn in (26, 6):
        out, st = M.post(a, [((1,), "fill", 0, 1)], conn)
        assert st.tolist() == [[1, 27]] and (out[2:7, 2:7, 2:7] == 1).all() and out.sum() == 125
    # a corner voxel of the shell removed: the leak is a diagonal step, which only the 26-neighbourhood of the holes takes
    # (the rules at connectivity 6); at connectivity 26 the holes are 6-connected and the cavity stays closed
    b = a.copy()
    b[2, 2, 2] = 0
    assert M.post(b, [((1,), "fill", 0, 1)], 26)[1].tolist() == [[1, 27]]
    out, st = M.post(b, [((1,), "fill", 0, 1)], 6)
    assert st.tolist() == [[0, 0]] and np.array_equal(out, b)
    # a hole holding another label is overwritten; with that label in the mask it is no hole
    c = a.copy()
    c[4, 4, 4] = 2
    out, st = M.post(c, [((1,), "fill", 0, 1)], 26)
    assert st.tolist() == [[1, 27]] and out[4, 4, 4] == 1
    out, st = M.post(c, [((1, 2), "fill", 0, 1)], 26)
    assert st.tolist() == [[1, 26]] and out[4, 4, 4] == 2 and out[3, 3, 3] == 1
    # an island of the mask inside the hole splits nothing: one hole of 26 voxels
    d = a.copy()
    d[4, 4, 4] = 1
    assert M.post(d, [((1,), "fill", 0, 1)], 26)[1].tolist() == [[1, 26]]
    # a hole touching a face is none; an axis of extent 1 leaves none; an empty and a full mask change nothing
    e = np.zeros((5, 5, 5), dtype=np.uint8)
    e[0:3, 1:4, 1:4] = 1
    e[0:2, 2, 2] = 0
    assert M.post(e, [((1,), "fill", 0, 1)], 26)[1].tolist() == [[0, 0]]
    f = np.ones((1, 5, 5), dtype=np.uint8)
    f[0, 2, 2] = 0
    assert M.post(f, [((1,), "fill", 0, 1)], 26)[1].tolist() == [[0, 0]]
    for v in (0, 1):
        g = np.full((3, 4, 5), v, dtype=np.uint8)
        out, st = M.post(g, [((1,), "fill", 0, 1)], 26)
        assert st.tolist() == [[0, 0]] and np.array_equal(out, g)


def test_restatement_closes_and_opens_on_the_infinite_grid():
    # a single voxel one step from a face: close3 leaves it alone (an unpadded closing grows it towards the face)
    a = np.zeros((9, 9, 9), dtype=np.uint8)
    a[1, 4, 4] = 1
    out, st = M.post(a, [((1,), "close", 3, 1)], 26)
    assert st.tolist() == [[1, 0]] and np.array_equal(out, a)
    out, st = M.post(a, [((1,), "open", 1, 0)], 26)
    assert st.tolist() == [[1, 1]] and out.sum() == 0
    # B_1 is the 7-voxel cross.  A 5 x 5 x 5 block without its centre: close1 gives the centre back and nothing else (the
    # dilation adds the six face layers without their rims, the erosion takes exactly those away again)
    b = np.zeros((9, 9, 9), dtype=np.uint8)
    b[2:7, 2:7, 2:7] = 1
    b[4, 4, 4] = 0
    out, st = M.post(b, [((1,), "close", 1, 1)], 26)
    assert st.tolist() == [[124, 1]] and out[4, 4, 4] == 1 and out.sum() == 125
    # a 3 x 3 x 3 block with a spur of three voxels along w: the erosion by the cross leaves the block's centre and the
    # voxel between it and the spur, the dilation gives back their two crosses, 12 voxels - the spur's first among them
    c = np.zeros((7, 7, 9), dtype=np.uint8)
    c[2:5, 2:5, 2:5] = 2
    c[3, 3, 5:8] = 2
    out, st = M.post(c, [((2,), "open", 1, 1)], 26)
    assert st.tolist() == [[30, 18]] and (out[3, 3, 6:8] == 1).all() and (out[3, 3, 2:6] == 2).all()
    assert out[2, 2, 2] == 1 and out[2, 3, 3] == 2 and int((out == 2).sum()) == 12
    rng = np.random.default_rng(5)
    for shape in ((7, 9, 11), (12, 10, 33), (5, 40, 6)):
        for dens in (0.15, 0.6):
            m = rng.random(shape) < dens
            for r in (1, 2, 3):
                cl, op = M.close(m, r), M.open_(m, r)
                assert (cl | m).sum() == cl.sum() and (op & m).sum() == op.sum()          # extensive, anti-extensive
                assert np.array_equal(M.close(cl, r), cl) and np.array_equal(M.open_(op, r), op)      # idempotent
                # the thresholds of the exact squared distance give the same sets: what the device computes, and
                # what the restatement uses beyond scipy's reach
                assert np.array_equal(M.close_by_distance(m, r), cl) and np.array_equal(M.open_by_distance(m, r), op)
                # an unpadded closing is another operation
                flat = M.ndimage.binary_closing(m, M.ball(r))
                assert not np.array_equal(flat, cl)
    for v in (0, 1):
        g = np.full((3, 4, 5), v, dtype=np.uint8)
        out, st = M.post(g, [((1,), "close", 2, 1), ((1,), "open", 2, 0)], 26)
        # the full volume is 3 voxels thick: no voxel is further than 2 from the outside, the opening takes it all
        assert np.array_equal(out, np.zeros_like(g)) and st.tolist() == [[60 * v, 0], [60 * v, 60 * v]]


def test_restatement_chains_old_and_new_rules_in_order():
    a = _shell()
    a[0, 0, 0] = 1                                   # a speck
    a[4, 4, 4] = 2
    rules = [((1,), "fill", 0, 1), ((1,), "largest", 0, 0), ((1,), "open", 1, 3)]
    out, st = M.post(a, rules, 26)
    assert st[0].tolist() == [1, 27] and st[1].tolist() == [2, 1] and st[2, 0] == 125
    assert out[0, 0, 0] == 0 and out[4, 4, 4] == 1 and out[2, 2, 2] == 3 and set(np.unique(out)) == {0, 1, 3}
