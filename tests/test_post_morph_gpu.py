"""effq_label_post on a real MI355X (-m gpu): holes filled and masks closed or opened by a ball, bit for bit - map and
stats - against the numpy / scipy restatement of tests/label_morph_ref.py.  Everything is integer, so no tolerance
appears anywhere.  The labelling tile is 8 x 8 x 32 and a row of the distance transform is walked in chunks of 64: the
shapes are the smallest that cross both in every axis."""
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from efficientq_amd import _lib, config as Cf, evaluate as E, nifti, predict, synth
from efficientq_amd.hip_ops import get_ops
from tests import label_clean_ref as R, label_morph_ref as M
from tests.test_prep_cpu import write_scan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3, 5, 33), (9, 17, 70), (17, 9, 65)]


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def _post(ops, a, rules, conn=26, inplace=False):
    m = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    before = m.clone()
    out, stats = ops.label_clean(m, rules, conn, out=m if inplace else None)
    assert out.dtype == torch.uint8 and out.shape == m.shape and stats.dtype == torch.int64
    assert stats.shape == (len(rules), 2) and (inplace or torch.equal(m, before))
    return out.cpu().numpy(), stats.cpu().numpy()


def _check(ops, a, rules, conn=26):
    got, stats = _post(ops, a, rules, conn)
    want, wstats = M.post(a, rules, conn)
    assert np.array_equal(got, want), f"{int((got != want).sum())} voxels differ for {rules} at {conn}"
    assert np.array_equal(stats, wstats), f"stats {stats.tolist()}, want {wstats.tolist()} for {rules} at {conn}"
    return got, stats


def _random_map(shape, seed, density):
    g = np.random.default_rng(seed)
    fg = g.random(shape) < density
    return np.where(fg, g.choice(np.array([1, 2, 4], dtype=np.uint8), size=shape), 0).astype(np.uint8)


def _blobs(shape, seed, seeds=0.01, radius=2):
    """Sparse seeds grown by a ball, each blob's voxels of label 1 or 2 by position: ragged masks with gaps and spurs."""
    g = np.random.default_rng(seed)
    grown = ndimage.binary_dilation(g.random(shape) < seeds, M.ball(radius))
    lab = np.where(g.random(shape) < 0.7, 1, 2).astype(np.uint8)
    return np.where(grown, lab, 0).astype(np.uint8)


def _shell(shape=(9, 9, 9), at=(2, 2, 2)):
    a = np.zeros(shape, dtype=np.uint8)
    d, h, w = at
    a[d:d + 5, h:h + 5, w:w + 5] = 1
    a[d + 1:d + 4, h + 1:h + 4, w + 1:w + 4] = 0
    return a


# ---- fill ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.3, 0.7, 0.92])
@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("shape", [(1, 1, 1)] + SHAPES)
def test_fill_of_random_maps_matches_the_restatement(ops, shape, conn, density):
    a = _random_map(shape, sum(shape) + conn, density)
    work = 0
    for labels, to in (((1,), 1), ((2, 4), 4), ((1, 2, 4), 2)):
        _, stats = _check(ops, a, [(labels, "fill", 0, to)], conn)
        work += int(stats[0, 1])
    # a sparse mask encloses little, least of all at connectivity 6, where the holes are 26-connected: the densest
    # maps carry the work
    assert work > 0 or density < 0.9 or min(shape) < 9


def test_fill_of_hand_made_cases(ops):
    # a hole that spans the corner of the labelling tiles at (8, 8, 32)
    a = np.ones((16, 16, 64), dtype=np.uint8)
    a[6:10, 6:10, 30:34] = 0
    a[0, 0, 0] = a[15, 15, 63] = 0                   # and two complement voxels on faces, which are none
    got, stats = _check(ops, a, [((1,), "fill", 0, 1)])
    assert stats.tolist() == [[1, 64]] and got[0, 0, 0] == 0 and (got[6:10, 6:10, 30:34] == 1).all()
    # the diagonal leak: closed at 26 (holes 6-connected), open at 6
    b = _shell()
    b[2, 2, 2] = 0
    assert _check(ops, b, [((1,), "fill", 0, 1)], 26)[1].tolist() == [[1, 27]]
    assert _check(ops, b, [((1,), "fill", 0, 1)], 6)[1].tolist() == [[0, 0]]
    assert _check(ops, _shell(), [((1,), "fill", 0, 1)], 6)[1].tolist() == [[1, 27]]
    # a hole touching a face, an island inside a hole, a hole holding another label (overwritten, or kept when it is
    # part of the mask), two holes in one map
    c = _shell((9, 12, 40), (0, 3, 30))
    c[0, 5, 32] = 0
    assert _check(ops, c, [((1,), "fill", 0, 1)])[1].tolist() == [[0, 0]]
    d = _shell()
    d[4, 4, 4] = 1
    assert _check(ops, d, [((1,), "fill", 0, 1)])[1].tolist() == [[1, 26]]
    e = _shell((9, 9, 40), (2, 2, 30))
    e[4, 4, 32] = 2
    e[2:7, 2:7, 2:7] = _shell()[2:7, 2:7, 2:7] * 2
    got, stats = _check(ops, e, [((1, 2), "fill", 0, 1)])
    assert stats.tolist() == [[2, 26 + 27]] and got[4, 4, 32] == 2 and got[4, 4, 4] == 1
    got, stats = _check(ops, e, [((1,), "fill", 0, 1)])
    assert stats.tolist() == [[1, 27]] and got[4, 4, 32] == 1 and got[4, 4, 4] == 0
    # an axis of extent 1, an empty and a full mask
    f = np.ones((1, 9, 70), dtype=np.uint8)
    f[0, 4, 30:40] = 0
    assert _check(ops, f, [((1,), "fill", 0, 1)])[1].tolist() == [[0, 0]]
    assert _check(ops, f.reshape(9, 1, 70), [((1,), "fill", 0, 1)])[1].tolist() == [[0, 0]]
    assert _check(ops, f.reshape(9, 70, 1), [((1,), "fill", 0, 1)])[1].tolist() == [[0, 0]]
    for v in (0, 1):
        g = np.full((9, 17, 70), v, dtype=np.uint8)
        got, stats = _check(ops, g, [((1,), "fill", 0, 1)])
        assert stats.tolist() == [[0, 0]] and np.array_equal(got, g)


# ---- close / open -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2, 3, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_close_and_open_match_the_restatement(ops, shape, radius):
    work = np.zeros(2, dtype=np.int64)
    for a in (_blobs(shape, sum(shape) + radius), _random_map(shape, radius, 0.8)):
        for labels, to in (((1,), 1), ((1, 2), 2)):
            work[0] += _check(ops, a, [(labels, "close", radius, to)])[1][0, 1]
        for labels, to in (((1,), 0), ((1, 2), 7)):
            work[1] += _check(ops, a, [(labels, "open", radius, to)])[1][0, 1]
    assert work.min() > 0, "the maps gave the rules nothing to do: the test shows nothing"


def test_the_widest_pad_at_a_small_size(ops):
    """R = 32 at (4, 6, 40): the padded plane is 68 x 70 x 104.  The restatement takes its sets from thresholds of the
    exact squared distance here (label_morph_ref.SCIPY_MAX_RADIUS)."""
    b = np.ones((4, 6, 40), dtype=np.uint8)
    b[1:3, 2:4, 10:30] = 0                           # a cavity is closed, a missing corner of the volume is not
    b[0, 0, 0] = 0
    got, stats = _check(ops, b, [((1,), "close", 32, 1)])
    assert stats.tolist() == [[879, 80]] and got[0, 0, 0] == 0
    got, stats = _check(ops, _random_map((4, 6, 40), 3, 0.5), [((1, 2), "close", 32, 1), ((4,), "open", 32, 0)])
    assert stats[:, 1].min() > 0


def test_close_and_open_on_the_infinite_grid_and_at_the_trivial_masks(ops):
    # a single voxel one step from a face stays what it is: an unpadded closing grows it towards the face
    for at in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (7, 4, 4), (4, 7, 4), (4, 4, 7)):
        a = np.zeros((9, 9, 9), dtype=np.uint8)
        a[at] = 1
        got, stats = _check(ops, a, [((1,), "close", 3, 1)])
        assert stats.tolist() == [[1, 0]] and np.array_equal(got, a)
        for border in (0, 1):                        # scipy's own closing without the pad, at either border value
            assert not np.array_equal(ndimage.binary_closing(a != 0, M.ball(3), border_value=border), a != 0)
    for shape in ((9, 17, 70), (3, 4, 5)):
        for v in (0, 1):
            g = np.full(shape, v, dtype=np.uint8)
            got, stats = _check(ops, g, [((1,), "close", 2, 1)])
            assert stats.tolist() == [[g.size * v, 0]] and np.array_equal(got, g)
            got, stats = _check(ops, g, [((1,), "open", 1, 0)])
            assert stats[0, 0] == g.size * v and (v == 0 or stats[0, 1] > 0)
    # a map whose rows are a multiple of four voxels and one whose rows are not take different load widths
    for shape in ((5, 6, 8), (5, 6, 7)):
        a = _random_map(shape, 11, 0.6)
        _check(ops, a, [((1, 2), "close", 1, 1)])
        _check(ops, a, [((1, 2), "open", 1, 0)])


# ---- chains -------------------------------------------------------------------------------------------------------------
CHAIN = [((1, 2), "fill", 0, 1), ((1, 2), "close", 2, 1), ((1, 2), "largest", 0, 0), ((2,), "open", 1, 1),
         ((2,), "min", 5, 1)]


def test_a_chain_of_old_and_new_rules_in_one_call(ops):
    a = _blobs((9, 17, 70), 21, seeds=0.015)
    assert [Cf.parse_post_rule(t) for t in ("1,2:fill>1", "1,2:close2>1", "1,2:largest", "2:open1>1", "2:min5>1")] == CHAIN
    got, stats = _check(ops, a, CHAIN)
    assert (stats[:, 1] > 0).sum() >= 3, stats.tolist()
    again, stats2 = _post(ops, a, CHAIN, inplace=True)
    assert np.array_equal(again, got) and np.array_equal(stats2, stats)              # in place equals out of place
    third, stats3 = _post(ops, a, CHAIN)
    assert np.array_equal(third, got) and np.array_equal(stats3, stats)              # two runs give equal bits
    _check(ops, a, CHAIN, 6)


def test_old_rules_through_effq_label_post_are_effq_label_cleans_bits(ops):
    old = [((1, 2), "largest", 0, 0), ((2,), "min", 5, 1), ((4,), "min", 2, 0)]
    a = _random_map((9, 17, 70), 8, 0.35)
    m = torch.from_numpy(a).to(DEV)
    want, wstats = ops.label_clean(m, old, 26)                                       # effq_label_clean
    sets = (C.c_uint8 * (256 * 3))()
    words = (C.c_longlong * 9)()
    for r, (labels, op, n, to) in enumerate(old):
        for v in labels:
            sets[256 * r + v] = 1
        words[3 * r:3 * r + 3] = [_lib.LABEL_CLEAN_OPS[op], n, to]
    D, H, W = a.shape
    for radius in (0, 2):                            # the workspace of a chain with a ball serves too
        need = ops.lib.effq_label_post_ws_bytes(D, H, W, radius)
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        out = torch.empty_like(m)
        stats = torch.full((3, 2), -1, dtype=torch.int64, device=DEV)
        rc = ops.lib.effq_label_post(m.data_ptr(), D, H, W, 26, 3, sets, words, out.data_ptr(), stats.data_ptr(),
                                     ws.data_ptr(), need, None)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(out, want) and torch.equal(stats, wstats)
    rw, rs = R.clean(a, old, 26)
    assert np.array_equal(want.cpu().numpy(), rw) and np.array_equal(wstats.cpu().numpy(), rs)


# ---- end to end -----------------------------------------------------------------------------------------------------------
AFFINE = np.array([[0.0, -1.0, 0.0, 20.0], [1.0, 0.0, 0.0, -7.0], [0.0, 0.0, 2.0, 3.0], [0.0, 0.0, 0.0, 1.0]])


def _scans(root, names):
    os.makedirs(os.path.join(root, "src"), exist_ok=True)
    lines = ["subject,ct"]
    for i, sn in enumerate(names):
        g = np.random.default_rng(60 + i)
        vol = np.zeros((40, 44, 36), dtype=np.int16)
        vol[3:-3, 3:-3, 1:-1] = g.integers(-400, 500, size=(34, 38, 34))
        write_scan(os.path.join(root, "src", f"{sn}.nii.gz"), vol, affine=AFFINE)
        lines.append(f"{sn},src/{sn}.nii.gz")
    with open(os.path.join(root, "cases.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return os.path.join(root, "cases.csv")


def _tiny_net(root=None):
    """A seeded random TINY_NET in full precision.  As it comes class 0 wins nearly everywhere; the last layer's bias of
    the classes 1 and 2 is raised until label 1 holds about a third of the scan with pockets of the others in it (holes
    to fill, ragged rims to open) and label 2 comes in specks (work for the rules of the old kind)."""
    args = Cf.make_args(dict(Cf.TINY_NET, qconv="conv"), 4, 4, merge_type=None)
    QConv, _, kwQ = Cf.get_conv_class(args)
    net = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
    synth.randomise_network(net, 0)
    head = [m for m in net.modules() if isinstance(m, torch.nn.Conv3d)][-1]
    assert head.out_channels == 3
    with torch.no_grad():
        head.bias[1] += 8.0
        head.bias[2] += 5.0
    path = None
    if root is not None:
        path = os.path.join(root, "state.pkl")
        torch.save({"state_dict": net.state_dict()}, path)
    return args, net, path


class _Calls:
    """Counts the calls of the two entry points through the handle's library."""

    def __init__(self, monkeypatch, ops):
        self.n = {"effq_label_clean": 0, "effq_label_post": 0}
        for name in self.n:
            monkeypatch.setattr(ops.lib, name, self._wrap(name, getattr(ops.lib, name)))

    def _wrap(self, name, fn):
        def call(*a):
            self.n[name] += 1
            return fn(*a)
        return call


def test_predict_with_the_new_rules_writes_the_restated_map_and_old_rules_take_the_old_path(tmp_path, ops, monkeypatch):
    root = str(tmp_path)
    lst = _scans(root, ["b", "a"])
    args, _, ckpt = _tiny_net(root)
    calls = _Calls(monkeypatch, ops)
    new, old = ["1:fill>1", "1:open1"], ["1:largest", "2:min4>1"]
    tables, seen = {}, {}
    for name, post in (("plain", None), ("new", new), ("old", old)):
        before = dict(calls.n)
        for k, v in dict(src_list=lst, out_dir=os.path.join(root, name), patch_size="32,32,32", prep_mask="nonzero",
                         pretrain=ckpt, post=post).items():
            setattr(args, k, v)
        predict.run(args, window_batch=1)
        seen[name] = {k: calls.n[k] - before[k] for k in calls.n}
        with open(os.path.join(root, name, predict.PREDICT_CSV), newline="") as f:
            tables[name] = list(csv.reader(f))
    # rules of the old kind make the calls they made, and no other
    assert seen == {"plain": {"effq_label_clean": 0, "effq_label_post": 0},
                    "new": {"effq_label_clean": 0, "effq_label_post": 2},
                    "old": {"effq_label_clean": 2, "effq_label_post": 0}}
    rules = {"new": [((1,), "fill", 0, 1), ((1,), "open", 1, 0)], "old": [((1,), "largest", 0, 0), ((2,), "min", 4, 1)]}
    said = {"new": "1:fill>1 1:open1", "old": "1:largest 2:min4>1"}
    assert tables["plain"][0] == predict.CSV_HEADER
    for name in ("new", "old"):
        assert tables[name][0] == predict.CSV_HEADER + predict.CSV_POST_COLUMNS
        total = np.zeros(2, dtype=np.int64)
        for r0, r1 in zip(tables["plain"][1:], tables[name][1:]):
            sn = r1[0]
            before, _ = nifti.read_nifti(os.path.join(root, "plain", f"{sn}.nii.gz"))
            after, _ = nifti.read_nifti(os.path.join(root, name, f"{sn}.nii.gz"))
            want, stats = M.post(before, rules[name], 26)
            assert after.dtype == np.uint8 and after.shape == (40, 44, 36) and np.array_equal(after, want)
            assert r1[-2] == said[name] and Cf.parse_post_text(r1[-2]) == (rules[name], 26)
            assert [int(v) for v in r1[-1].split()] == stats[:, 1].tolist()
            k = predict.CSV_HEADER.index("labels")
            assert r0[:k] == r1[:k]
            count = np.bincount(after.ravel())
            assert [int(v) for v in r1[k].split()] == [v for v in range(len(count)) if count[v]]
            assert [int(v) for v in r1[k + 1].split()] == [int(n) for n in count if n]
            total += stats[:, 1]
        assert total.min() > 0, "the maps gave a rule nothing to do: the test shows nothing"


def test_validate_seg_scores_the_filled_map(tmp_path, ops):
    _, net, _ = _tiny_net()
    net = net.to(DEV).eval()
    g = torch.Generator().manual_seed(4)
    shape = (20, 24, 18)
    loader = [(torch.randn(1, 1, *shape, generator=g), torch.randint(0, 3, (1,) + shape, generator=g)) for _ in range(2)]
    rules = [((1, 2), "fill", 0, 1), ((2,), "open", 1, 1)]
    kw = dict(task="lits", patch_size=(16, 16, 16), overlap=(4, 4, 4), window_batch=2, names=["s1", "s2"])
    with torch.no_grad():
        base = E.validate_seg(net, loader, **kw)
        res = E.validate_seg(net, loader, post=rules, **kw)
        path = os.path.join(str(tmp_path), "metrics_post.csv")
        E.write_metrics_post_csv(path, res)
        with open(path, newline="") as f:
            table = list(csv.reader(f))
        assert table[0] == ["subject", "class", "dsc", "sens", "spec", "acc", "tp", "fp", "fn", "tn", "changed_0", "changed_1"]
        work = 0
        for r0, r, (img, lab) in zip(base, res, loader):
            assert all(torch.equal(r0[k], r[k]) for k in ("counts",) + E.METRICS)
            logits, _, _ = E.stitched_window_logits(ops, [net], img.to(DEV), (16, 16, 16), (4, 4, 4), 2)
            pmap = logits[0][0].argmax(0).cpu().numpy().astype(np.uint8)
            want, stats = M.post(pmap, rules, 26)
            counts = R.tallies(want, lab[0].numpy().astype(np.uint8), R.class_lut("argmax", 3), 3)
            rows = [row for row in table[1:] if row[0] == r["name"]]
            assert [[int(v) for v in row[6:10]] for row in rows] == counts.tolist()
            assert all([int(v) for v in row[10:]] == stats[:, 1].tolist() for row in rows)
            assert r["post"]["counts"].tolist() == counts.tolist() and r["post"]["changed"] == stats[:, 1].tolist()
            work += int(stats[:, 1].min())
        assert work > 0, "the maps gave a rule nothing to do: the test shows nothing"
