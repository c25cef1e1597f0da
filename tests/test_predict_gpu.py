"""The `predict` mission on a real MI355X (-m gpu): effq_seg_labels_source against the fp64 restatement of
test_predict_cpu, the snapshot round trip of calibrate.load_calibrated, and the mission end to end.

The bar of the kernel test.  The kernel interpolates in fp32 with fp32 weights, the restatement in fp64 with fp64
weights; a label may differ only where the fp64 values are so close to deciding otherwise that fp32 rounding can tip
them.  With M the largest |logit| of the case (no corner is larger) one level  l0 a + l1 b  of the interpolation errs by
at most: the two weights, each within 2^-25 of the fp64 weight (l1 is one rounding of q - i0 < 1, and 1.0f - l1 is exact
or one more rounding of a number below 1), times |a|, |b| <= M: 2 * 2^-25 M; the two products, each rounded once, 2^-24
relative of l0 |a| and l1 |b|, which sum to at most M: 2^-24 M; the sum, rounded once: 2^-24 M.  That is 3 * 2^-24 M
per level, and the errors of a level pass through the next with weights that sum to 1, so the three levels give
9 * 2^-24 M plus second-order terms: BOUND = 16 * 2^-24 * M holds it with room.  In argmax mode two channels move, so the
gap of the two largest is compared with 2 BOUND; in the sigmoid rules each channel is compared with the threshold, at
BOUND.  Voxels inside the box whose fp64 margin is at most that are excluded from the comparison; their share is
computed from the restatement alone and must not exceed 1e-3 of the voxels inside (expected about 1e-5: the density of
the margin near 0 is about 0.1 per unit for logits of 4 N(0, 1), the bound about 2e-5 wide; a box of one voxel holds at
most a few dozen source voxels and must have none).  Everywhere else, and outside the box (label 0), the maps must be
equal.  The bound is derived, not measured."""
import csv
import os

import numpy as np
import pytest
import torch

from efficientq_amd import _lib, calibrate as K, config as Cf, data as D, evaluate as E, nifti, predict, prep, synth
from efficientq_amd.hip_ops import get_ops
from tests.test_predict_cpu import ref_labels_source
from tests.test_prep_cpu import write_scan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RULES = [("argmax", None), ("brats", "con"), ("brats", "agg"), ("brats", None), ("rank", "con")]
SOURCES = [(1, 1, 1), (19, 23, 37), (40, 44, 65)]
FACTORS = [(1.0, 1.0, 1.0), (0.64, 1.37, 2.5), (2.0, 0.5, 1.0)]
CLASSES = [1, 2, 3, 4, 8]
EXCLUDED_SHARE_MAX = 1e-3


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def _boxes(G):
    """(pmin, extent): the whole grid, a box touching the low corner, one touching the high corner, and an interior box
    of one voxel per axis."""
    half = tuple(max(1, (n + 1) // 2) for n in G)
    return [((0, 0, 0), tuple(G)), ((0, 0, 0), half), (tuple(n - h for n, h in zip(G, half)), half),
            (tuple(n // 2 for n in G), (1, 1, 1))]


def _compare(ops, logits, pmin, G, factors, source, rule, fuse, tag):
    """One launch against the restatement at the bar of the module docstring; returns (excluded, inside)."""
    want, margin, inside = ref_labels_source(logits.numpy(), pmin, G, factors, source, rule, fuse, ops.sigmoid_threshold())
    bound = 16.0 * 2.0 ** -24 * float(logits.abs().max()) * (2.0 if rule == "argmax" else 1.0)
    unsure = inside & (margin <= bound)
    n_in, n_ex = int(inside.sum()), int(unsure.sum())
    print(f"{tag}: {n_in} voxels inside, {n_ex} excluded (margin <= {bound:.3g})")
    assert n_ex <= EXCLUDED_SHARE_MAX * n_in, tag           # from the restatement alone, before the kernel runs
    got = ops.seg_labels_source(logits.to(DEV), pmin, G, factors, source, rule, fuse)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(source)
    got = got.cpu().numpy()
    assert not got[~inside].any(), tag
    sure = ~unsure
    assert np.array_equal(got[sure], want[sure]), tag
    return n_ex, n_in


@pytest.mark.parametrize("factors", FACTORS)
@pytest.mark.parametrize("source", SOURCES)
def test_source_labels_against_the_fp64_restatement(ops, source, factors):
    G = tuple(prep.resample_extent(n, f) for n, f in zip(source, factors))
    excluded = inside = 0
    for b, (pmin, ext) in enumerate(_boxes(G)):
        for Cc in CLASSES:
            seed = 1000 * SOURCES.index(source) + 100 * FACTORS.index(factors) + 10 * b + Cc
            logits = 4.0 * torch.randn((Cc,) + ext, generator=torch.Generator().manual_seed(seed))
            for rule, fuse in RULES:
                if rule == "brats" and Cc < 3:
                    continue
                ex, n = _compare(ops, logits, pmin, G, factors, source, rule, fuse,
                                 f"source {source} f {factors} box {pmin}+{ext} C {Cc} {rule}/{fuse}")
                excluded, inside = excluded + ex, inside + n
    print(f"source {source} f {factors}: {excluded} of {inside} inside voxels excluded over all boxes, classes and rules")
    assert inside > 0


@pytest.mark.parametrize("Cc", [3, 4])
def test_dyadic_ties_are_decided_as_the_restatement_decides_them(ops, Cc):
    """Logits that are multiples of 0.25 with many equal channels, factors (0.5, 1, 0.5): every weight is 0, 0.5 or 1 and
    every product and sum is exact in fp32 and in fp64, so nothing is excluded: the first maximum wins a tie, and a value
    equal to the threshold's side is decided as v >= thresh decides it."""
    source, factors = (10, 9, 12), (0.5, 1.0, 0.5)
    G = (20, 9, 24)
    pmin, ext = (3, 1, 2), (13, 7, 20)
    g = torch.Generator().manual_seed(11 + Cc)
    logits = torch.randint(-3, 4, (Cc,) + ext, generator=g).float() * 0.25
    thresh = ops.sigmoid_threshold()
    ties = 0
    for rule, fuse in RULES:
        want, margin, inside = ref_labels_source(logits.numpy(), pmin, G, factors, source, rule, fuse, thresh)
        got = ops.seg_labels_source(logits.to(DEV), pmin, G, factors, source, rule, fuse).cpu().numpy()
        assert np.array_equal(got, want), (rule, fuse)
        ties += int((margin[inside] == 0).sum()) if rule == "argmax" else 0
        assert 0 < inside.sum() < inside.size
    assert ties > 10                                         # the tie rule was exercised


@pytest.mark.parametrize("factors", [None, (1.0, 1.0, 1.0)])
def test_identity_factors_equal_the_restored_crop_of_seg_labels(ops, factors):
    source = (19, 23, 37)
    pmin, pmax = (3, 0, 5), (15, 23, 37)
    ext = tuple(b - a for a, b in zip(pmin, pmax))
    logits = (4.0 * torch.randn((4,) + ext, generator=torch.Generator().manual_seed(21))).to(DEV)
    logits.view(-1)[::5] = torch.round(logits.view(-1)[::5])          # ties among the channels
    for rule, fuse in RULES + [("rank", None), ("rank", "agg")]:
        want = D.restore_crop(ops.seg_labels(logits[None], rule, fuse)[0].cpu().numpy(), pmin, pmax, source)
        got = ops.seg_labels_source(logits, pmin, source, factors, source, rule, fuse).cpu().numpy()
        assert got.tobytes() == want.tobytes(), (rule, fuse)


def test_source_labels_are_deterministic(ops):
    source, factors = (40, 44, 65), (0.64, 1.37, 2.5)
    G = tuple(prep.resample_extent(n, f) for n, f in zip(source, factors))
    logits = (4.0 * torch.randn((3,) + G, generator=torch.Generator().manual_seed(31))).to(DEV)
    for rule, fuse in (("argmax", None), ("brats", "con")):
        a = ops.seg_labels_source(logits, (0, 0, 0), G, factors, source, rule, fuse)
        b = ops.seg_labels_source(logits, (0, 0, 0), G, factors, source, rule, fuse)
        assert torch.equal(a, b) and int(a.max()) > 0


def test_source_labels_refuse_bad_arguments_before_any_launch(ops):
    x = torch.randn(3, 4, 5, 6, device=DEV)
    ok = ((0, 0, 0), (4, 5, 6), (1.0, 1.0, 1.0), (4, 5, 6))
    assert ops.seg_labels_source(x, *ok, "argmax").shape == (4, 5, 6)
    with pytest.raises(_lib.EffqError):
        ops.seg_labels_source(x, *ok, "planes")                                   # no planes on a source grid
    with pytest.raises(_lib.EffqError):
        ops.seg_labels_source(torch.randn(9, 4, 5, 6, device=DEV), *ok, "rank")   # the class limit
    with pytest.raises(_lib.EffqError):
        ops.seg_labels_source(x, (1, 0, 0), (4, 5, 6), (1.0, 1.0, 1.0), (4, 5, 6), "argmax")     # pmin + g > G
    with pytest.raises(_lib.EffqError):
        ops.seg_labels_source(x, (0, 0, 0), (4, 5, 6), (1.0, 0.0, 1.0), (4, 5, 6), "argmax")     # a zero factor
    with pytest.raises(_lib.EffqError):
        ops.seg_labels_source(x, (0, 0, 0), (4, 5, 6), (1.0, 1.0, float("nan")), (4, 5, 6), "argmax")
    with pytest.raises(_lib.EffqError):
        ops.seg_labels_source(x, (0, 0, 0), (4, 5, 6), (1.0, 1.0, 1.0), (4, 40000, 6), "argmax")  # an extent of 40000
    with pytest.raises(_lib.EffqError):
        ops.seg_labels_source(x, (0, 0, 0), (4, 40000, 6), (1.0, 1.0, 1.0), (4, 5, 6), "argmax")
    with pytest.raises(_lib.EffqError):
        ops.seg_labels_source(x[:2], *ok[:1], (2, 5, 6), *ok[2:], "brats", "con")  # brats needs three channels
    with pytest.raises(_lib.EffqError):
        ops.seg_labels_source(x, *ok, "argmax", "con")                            # a merge needs a sigmoid rule
    # the entry point itself, past the wrapper's own checks: a source extent of 40000, a null pointer, the planes rule
    import ctypes as C
    from efficientq_amd.hip_ops import _ptr
    i3, d3, ERR_ARG = C.c_int * 3, C.c_double * 3, 1            # include/effq_hip.h: EFFQ_ERR_ARG
    out = torch.zeros(4 * 5 * 6, dtype=torch.uint8, device=DEV)

    def raw(source=(4, 5, 6), rule=0, logits=x, box=(4, 5, 6)):
        return ops.lib.effq_seg_labels_source(_ptr(logits), 3, i3(*box), i3(0, 0, 0), i3(4, 5, 6), d3(1.0, 1.0, 1.0),
                                              i3(*source), rule, 0, 0.0, _ptr(out), ops.stream)
    assert raw() == 0
    assert raw(source=(4, 40000, 6)) == ERR_ARG and raw(source=(4, 0, 6)) == ERR_ARG
    assert raw(rule=_lib.SEG_LABEL_RULES["planes"]) == ERR_ARG and raw(logits=None) == ERR_ARG
    assert raw(box=(4, 5, 40000)) == ERR_ARG
    torch.cuda.synchronize()                                                     # nothing faulted on the way
    assert int(out.max()) <= 2


# ---- the snapshot round trip ------------------------------------------------------------------------------------------
def _net(width="8,16,8", channel=False):
    args = Cf.make_args(dict(Cf.TINY_NET, width=width), 4, 4, lwq_batchsz=2, lwq_channel_wise=channel)
    QConv, _, kwQ = Cf.get_conv_class(args)
    return args, Cf.get_model_cube(args, QConv, kwQ)[0]["model"]


def _calibrated(root, channel):
    """TINY_NET calibrated at 4 / 4 levels on two synthetic 32^3 volumes, its last-head logits on a held-out volume, and
    the three snapshots written the way do_ptq ends."""
    from efficientq_amd.entrance import _SnapshotWriter
    args, model = _net(channel=channel)
    synth.randomise_network(model, 0)
    model.eval()
    K.search_fold_and_remove_bn(model)
    model.to(DEV)
    K.set_name(model)
    K.calibrate_model(model, synth.calib_batch("lits", range(2), 32).to(DEV), "lits", args.init_stride)
    K.set_quantized(model)
    held = synth.calib_batch("lits", [2], 32).to(DEV)
    with torch.no_grad():
        logits = E._last_head(model(held)).clone()
    os.makedirs(root, exist_ok=True)
    model.cpu()
    w = _SnapshotWriter(model, root)
    w.snapshot("state_in_fp.pkl")
    K.store_int_weight(model)
    w.snapshot("state_in_int8.pkl")
    w.snapshot("state_in_int8_compress.npz", compress=True)
    return held, logits


@pytest.fixture(scope="module")
def snap_tensor(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("snap_tensor"))
    return (root,) + _calibrated(root, False)


@pytest.fixture(scope="module")
def snap_channel(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("snap_channel"))
    return (root,) + _calibrated(root, True)


def _logits_of(path, held, channel):
    model = K.load_calibrated(_net(channel=channel)[1], path, DEV)
    with torch.no_grad():
        return model, E._last_head(model(held))


def test_fp_snapshot_gives_the_calibrated_logits_bit_for_bit(snap_tensor, capsys):
    root, held, want = snap_tensor
    assert sorted(os.listdir(root)) == ["state_in_fp.pkl", "state_in_int8.pkl", "state_in_int8_compress.npz"]
    _, got = _logits_of(os.path.join(root, "state_in_fp.pkl"), held, False)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert "Q6" not in capsys.readouterr().out


def test_channel_mode_snapshots_give_the_calibrated_logits_bit_for_bit(snap_channel, capsys):
    root, held, want = snap_channel
    for name in ("state_in_fp.pkl", "state_in_int8.pkl"):
        _, got = _logits_of(os.path.join(root, name), held, True)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), name
    assert "Q6" not in capsys.readouterr().out


def test_per_tensor_int8_snapshot_restores_the_grid_of_alpha_w_and_says_so(snap_tensor, capsys):
    root, held, _ = snap_tensor
    path = os.path.join(root, "state_in_int8.pkl")
    model, got = _logits_of(path, held, False)
    out = capsys.readouterr().out
    assert len([ln for ln in out.splitlines() if "Q6" in ln and "state_in_fp.pkl" in ln]) == 1
    sd = torch.load(path, map_location="cpu")["state_dict"]
    convs = list(K._each_q(model))
    assert convs and torch.isfinite(got).all()
    for name, q in convs:
        ids = sd[name + ".weight"]
        assert ids.dtype == torch.uint8
        want = sd[name + ".alpha_w"] * (ids.float() * (2 / (q.qlvl_w - 1)) - 1)
        assert torch.equal(q.weight.data.cpu(), want), name
        assert q._quantized and q.weight.device.type == "cuda"


def test_a_snapshot_of_another_network_is_refused_by_key(tmp_path, capsys):
    _, wide = _net("16,32,16")
    wide.eval()
    K.search_fold_and_remove_bn(wide)
    path = str(tmp_path / "state_in_fp.pkl")
    torch.save({"state_dict": wide.state_dict()}, path)
    _, model = _net()
    with pytest.raises(SystemExit) as e:
        K.load_calibrated(model, path, DEV)
    keys = list(model.state_dict())
    assert "--resume" in str(e.value) and any(k in str(e.value) for k in keys)
    # keys that do not fit at all: the first missing and the first unexpected are named
    torch.save({"state_dict": {"nothing.weight": torch.zeros(1)}}, path)
    with pytest.raises(SystemExit) as e:
        K.load_calibrated(_net()[1], path, DEV)
    assert keys[0] in str(e.value) and "nothing.weight" in str(e.value)
    assert os.listdir(str(tmp_path)) == ["state_in_fp.pkl"]


# ---- the mission end to end ---------------------------------------------------------------------------------------------
AFFINE = np.array([[0.0, -1.0, 0.0, 20.0], [1.0, 0.0, 0.0, -7.0], [0.0, 0.0, 2.0, 3.0], [0.0, 0.0, 0.0, 1.0]])


def _scans(root, names):
    os.makedirs(os.path.join(root, "src"), exist_ok=True)
    lines = ["subject,ct"]
    for i, sn in enumerate(names):
        g = np.random.default_rng(40 + i)
        vol = np.zeros((40, 44, 36), dtype=np.int16)
        vol[3:-3, 3:-3, 1:-1] = g.integers(-400, 500, size=(34, 38, 34))
        write_scan(os.path.join(root, "src", f"{sn}.nii.gz"), vol, affine=AFFINE)
        lines.append(f"{sn},src/{sn}.nii.gz")
    with open(os.path.join(root, "cases.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return os.path.join(root, "cases.csv")


@pytest.mark.parametrize("spacing", [None, "1.2,1.25,2"])
def test_mission_end_to_end(ops, snap_tensor, tmp_path, spacing):
    root, out = str(tmp_path), str(tmp_path / "seg")
    lst = _scans(root, ["b", "a"])
    resume = os.path.join(snap_tensor[0], "state_in_fp.pkl")
    args, _ = _net()
    for k, v in dict(src_list=lst, out_dir=out, patch_size="32,32,32", prep_spacing=spacing, prep_mask="nonzero",
                     resume=resume, merge_type=None).items():
        setattr(args, k, v)
    rows = predict.run(args, window_batch=1)
    assert [r["subject"] for r in rows] == ["a", "b"]
    table = list(csv.DictReader(open(os.path.join(out, predict.PREDICT_CSV))))
    model = K.load_calibrated(_net()[1], resume, DEV)
    sp = prep._triple(spacing, "spacing") if spacing else None
    patch, overlap = (32, 32, 32), (16, 16, 16)
    for r, entry in zip(table, prep.read_src_list(lst, "lits")):
        sn = r["subject"]
        plan = prep._Plan(entry, ("ct",), sp, patch)
        imgs = {"ct": nifti.read_image(entry["images"]["ct"])[0]}
        y, _, _, pmin, pmax, _, _, _ = prep.process_subject(
            ops, plan, imgs, None, ("ct",), prep.PrepOptions("nonzero", (-200.0, 250.0), sp, patch, False))
        vol = torch.from_numpy(y)[None].to(DEV)
        outs, nwin, _ = E.stitched_window_logits(ops, [model], vol, patch, overlap, 1)
        want = ops.seg_labels_source(outs[0][0], pmin, plan.grid_shape, plan.factors, plan.source_shape, "argmax")
        want = want.cpu().numpy()
        got, h = nifti.read_nifti(os.path.join(out, f"{sn}.nii.gz"))
        assert got.dtype == np.uint8 and got.shape == (40, 44, 36) and np.array_equal(got, want)
        assert np.allclose(h["affine"], AFFINE) and h["sform_code"] == 2
        assert plan.grid_shape == ((40, 44, 36) if spacing is None else (33, 35, 36)) and min(plan.grid_shape) >= 32
        assert r["grid_shape"] == prep._fmt(plan.grid_shape) and r["pmin"] == prep._fmt(pmin) and int(r["windows"]) == nwin
        assert r["prep_spacing"] == ("none" if spacing is None else "1.2 1.25 2") and r["patch_size"] == "32 32 32"
        count = np.bincount(got.ravel())
        labels = [int(v) for v in r["labels"].split()]
        assert labels == [v for v in range(len(count)) if count[v]] and len(labels) > 1
        assert [int(v) for v in r["voxels"].split()] == [int(count[v]) for v in labels]
        assert [float(v) for v in r["volume_ml"].split()] == pytest.approx([count[v] * 2.0 / 1000 for v in labels], rel=1e-6)
        if spacing is None:           # the map validate_seg writes on the source grid for the same subject, model and box
            geo = [{"spacing": plan.source_spacing, "header": plan.header, "pmin": pmin, "pmax": pmax,
                    "source_shape": plan.source_shape}]
            label = torch.zeros((1,) + tuple(y.shape[1:]), dtype=torch.uint8)
            E.validate_seg(model, [(torch.from_numpy(y)[None], label)], "lits", patch, overlap, window_batch=1,
                           names=[sn], save_dir=os.path.join(root, "val"), label_dtype=np.uint8, geometry=geo)
            val, hv = nifti.read_nifti(os.path.join(root, "val", f"{sn}.nii.gz"))
            assert np.array_equal(val, got) and np.allclose(hv["affine"], h["affine"])
