"""Gaussian window blending and mirror test-time augmentation on a real MI355X (-m gpu): the mirrored gather, the put
and the weighted stitch against torch and against the fp64 restatement of tests/test_window_blend_cpu.py, the window
function end to end with toy modules, validate_seg, and what the ops refuse.

Geometry: N = 2, volume (20, 18, 23), windows (8, 6, 10), overlap (3, 2, 4): 4 x 4 x 4 windows, the last of every axis
flush with the border one to four voxels after its neighbour, so the coverage counts are uneven (1 .. 18).  And a
volume that is one window.  C in 1, 3, 4, 8: the scalar and the 16-byte path of the gather and the put, and the full
unroll of the stitch."""
import numpy as np
import pytest
import torch

from efficientq_amd import _lib, evaluate as E
from efficientq_amd.hip_ops import blend_weights_host, from_ndhwc, get_ops
from tests.test_window_blend_cpu import blend_bound, ref_blend, ref_unflip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, VOL, P, O = 2, (20, 18, 23), (8, 6, 10), (3, 2, 4)
NWIN = 64
CHANNELS = [1, 3, 4, 8]


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def _dims(flip, first=1):
    """The tensor axes a flip mask mirrors when d is axis `first`."""
    return [first + b for b in range(3) if flip >> b & 1]


def _flip(t, flip, first=1):
    d = _dims(flip, first)
    return torch.flip(t, d) if d else t


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ---- gather, mirrored -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CHANNELS)
def test_gather_with_a_flip_mask_equals_the_flipped_gather_bitwise(ops, C):
    g = torch.Generator().manual_seed(C)
    for shape in (VOL, P):
        vol = torch.randn(N, C, *shape, generator=g).to(DEV)
        vol[0, 0, 0, 0, 0] = -0.0
        plain = ops.window_gather(vol, P, O)
        assert plain.shape[0] == (NWIN if shape == VOL else 1) * N
        for flip in range(8):
            got = ops.window_gather(vol, P, O, flip=flip)
            assert _same_bits(got, _flip(plain, flip)), (shape, flip)
        assert _same_bits(ops.window_gather(vol, P, O, flip=0), plain)
    # a sub-range of the windows (vol is the one-window volume now: take the large one again)
    vol = torch.randn(N, C, *VOL, generator=g).to(DEV)
    plain = ops.window_gather(vol, P, O)
    for flip in (0, 3, 7):
        part = ops.window_gather(vol, P, O, 5, 7, flip)
        assert _same_bits(part, _flip(plain[5 * N:12 * N], flip)), flip
    last = ops.window_gather(vol, P, O, NWIN - 1, 1, 5)
    assert _same_bits(last, _flip(plain[(NWIN - 1) * N:], 5))


# ---- put --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CHANNELS)
def test_put_transposes_unmirrors_and_stores_or_adds_bitwise(ops, C):
    g = torch.Generator().manual_seed(20 + C)
    M, lo = 5, 3                    # the slice: windows 3 .. 7 of a buffer of 11 (an offset of 3 * 480 * C floats)
    for flip in range(8):
        src = (4.0 * torch.randn(M, C, *P, generator=g)).to(DEV)
        src[0, 0, 0, 0, 0] = -0.0
        was = torch.randn(11, *P, C, generator=g).to(DEV)
        want = _flip(src.permute(0, 2, 3, 4, 1), flip)
        buf = was.clone()
        ops.window_put(src, buf[lo:lo + M], flip, False)
        assert _same_bits(buf[lo:lo + M], want), flip
        assert _same_bits(buf[:lo], was[:lo]) and _same_bits(buf[lo + M:], was[lo + M:]), flip
        buf = was.clone()
        ops.window_put(src, buf[lo:lo + M], flip, True)
        assert _same_bits(buf[lo:lo + M], was[lo:lo + M] + want), flip          # one fp32 add: nothing to reorder
        assert _same_bits(buf[:lo], was[:lo]) and _same_bits(buf[lo + M:], was[lo + M:]), flip
    # a slice that is not 16-byte aligned takes the scalar path whatever C is
    flat = torch.zeros(1 + 2 * 480 * C, device=DEV)
    src = torch.randn(2, C, *P, generator=g).to(DEV)
    ops.window_put(src, flat[1:].view(2, *P, C), 6, False)
    assert _same_bits(flat[1:].view(2, *P, C), _flip(src.permute(0, 2, 3, 4, 1), 6)) and float(flat[0]) == 0.0


@pytest.mark.parametrize("C", [3, 4])
def test_put_takes_a_channels_last_head_and_stores_it_unmirrored_without_allocating(ops, C):
    # what the convs of the package return: N x C x pd x ph x pw over channels-last storage (from_ndhwc)
    g = torch.Generator().manual_seed(30 + C)
    stored = (4.0 * torch.randn(5, *P, C, generator=g)).to(DEV)
    head = from_ndhwc(stored)
    assert not head.is_contiguous()
    was = torch.randn(5, *P, C, generator=g).to(DEV)
    buf = was.clone()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    ops.window_put(head, buf, 0, False)
    assert torch.cuda.max_memory_allocated(DEV) == base         # the default run's store sizes no window batch
    assert _same_bits(buf, stored)
    for flip, acc in ((0, True), (5, False), (5, True)):
        buf = was.clone()
        ops.window_put(head, buf, flip, acc)
        want = _flip(stored, flip)
        assert _same_bits(buf, was + want if acc else want), (flip, acc)


# ---- weighted stitch --------------------------------------------------------------------------------------------------------
def _weights_dev(kind):
    return tuple(torch.from_numpy(w).to(DEV) for w in blend_weights_host(P, kind))


@pytest.mark.parametrize("C", CHANNELS)
def test_weighted_stitch_with_ones_equals_the_stitch_bitwise(ops, C):
    g = torch.Generator().manual_seed(40 + C)
    for shape in (VOL, P):
        nwin = NWIN if shape == VOL else 1
        win = (3.0 * torch.randn(nwin * N, *P, C, generator=g)).to(DEV)
        win[0, 0, 0, 0, 0] = -0.0
        full = (N, C) + shape
        want = ops.window_stitch(win, full, P, O)
        assert _same_bits(ops.window_stitch(win, full, P, O, ops.blend_weights(P, "uniform"), 1), want)
    got = ops.blend_weights(P, "gauss")
    assert all(_same_bits(a, b) for a, b in zip(got, _weights_dev("gauss"))) and got[0].device.type == "cuda"


@pytest.mark.parametrize("nflip", [1, 8])
@pytest.mark.parametrize("C", CHANNELS)
def test_stitch_without_weights_equals_the_stitch_with_ones_bitwise_at_any_nflip(ops, C, nflip):
    # the two instances of the kernel: 1.0f * x is x and the weight sum is the exact count (18 at most here), so the
    # unweighted one - the route of uniform blending with mirror passes - divides by the same nflip * count
    g = torch.Generator().manual_seed(50 + C)
    for shape in (VOL, P):
        nwin = NWIN if shape == VOL else 1
        win = (3.0 * torch.randn(nwin * N, *P, C, generator=g)).to(DEV)
        win[0, 0, 0, 0, 0] = -0.0
        full = (N, C) + shape
        ones = ops.blend_weights(P, "uniform")
        assert _same_bits(ops.window_stitch(win, full, P, O, None, nflip), ops.window_stitch(win, full, P, O, ones, nflip))


@pytest.mark.parametrize("nflip", [1, 8])
@pytest.mark.parametrize("C", CHANNELS)
def test_weighted_stitch_against_the_fp64_restatement(ops, C, nflip):
    g = torch.Generator().manual_seed(60 + C)
    w = blend_weights_host(P, "gauss")
    for shape in (VOL, P):
        nwin = NWIN if shape == VOL else 1
        win = 4.0 * torch.randn(nwin * N, *P, C, generator=g)
        full = (N, C) + shape
        got = ops.window_stitch(win.to(DEV), full, P, O, _weights_dev("gauss"), nflip).cpu().numpy()
        ref, mag, cover = ref_blend([win.numpy()], w, full, P, O)
        ref, mag = ref / nflip, mag / nflip               # win holds the sum of nflip passes
        assert cover.max() == (18 if shape == VOL else 1) and cover.min() == 1
        err, bound = np.abs(got - ref), blend_bound(mag, cover[None, None])
        print(f"C={C} nflip={nflip} {shape}: max err/bound {np.max(err / bound):.3f}")
        assert (err <= bound).all()


def test_weighted_stitch_lets_the_weights_decide_not_the_counts(ops):
    # one spike at the corner voxel of one window: where that window's weight is least, the spike all but vanishes
    C, full = 3, (N, 3) + VOL
    win = torch.zeros(NWIN * N, *P, C)
    k = (1 * 16 + 1 * 4 + 1) * N            # window (1, 1, 1), starts (5, 4, 6), n = 0
    win[k, 0, 0, 0, 1] = 1e6                # its corner: volume voxel (5, 4, 6), also covered by window (0, 0, 0)
    w = blend_weights_host(P, "gauss")
    got = ops.window_stitch(win.to(DEV), full, P, O, _weights_dev("gauss"), 1).cpu().numpy()
    ref, mag, cover = ref_blend([win.numpy()], w, full, P, O)
    assert (np.abs(got - ref) <= blend_bound(mag, cover[None, None])).all()
    assert cover[5, 4, 6] == 8
    uniform = ops.window_stitch(win.to(DEV), full, P, O).cpu().numpy()
    assert uniform[0, 1, 5, 4, 6] == 1e6 / 8
    assert 0 < got[0, 1, 5, 4, 6] < 1e6 / 8 / 50 and np.count_nonzero(got) == 1


# ---- the window function end to end -----------------------------------------------------------------------------------------
def _conv(cin, cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.nn.Conv3d(cin, cout, k, padding=k // 2)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) / (cin * k ** 3) ** 0.5)
        m.bias.copy_(torch.randn(cout, generator=g))
    return m.eval()


def _parent_path(ops, net, vol, wb):
    """The window function as it was: window_gather, copy_, window_stitch.  Returns (stitched, the window buffer)."""
    buf = None
    for first in range(0, NWIN, wb):
        cnt = min(wb, NWIN - first)
        last = net(from_ndhwc(ops.window_gather(vol, P, O, first, cnt)))
        if buf is None:
            buf = torch.empty(NWIN * N, *P, int(last.shape[1]), device=DEV)
        buf[first * N:(first + cnt) * N].copy_(last.permute(0, 2, 3, 4, 1))
    return ops.window_stitch(buf, (N, int(buf.shape[-1])) + VOL, P, O), buf


@pytest.fixture(scope="module")
def volume():
    return torch.randn(N, 2, *VOL, generator=torch.Generator().manual_seed(7))


@torch.no_grad()
def test_defaults_give_the_bits_of_the_parent_path_and_two_nets_those_of_each_alone(ops, volume):
    vol = volume.to(DEV)
    a, b = _conv(2, 3, 3, 1).to(DEV), _conv(2, 3, 1, 2).to(DEV)       # one class count: one output shape
    outs, nwin, bsz = E.stitched_window_logits(ops, [a, b], vol, P, O, 24)
    assert (nwin, bsz) == (NWIN, 24)
    assert _same_bits(outs[0], _parent_path(ops, a, vol, 24)[0]) and _same_bits(outs[1], _parent_path(ops, b, vol, 24)[0])
    both, _, _ = E.stitched_window_logits(ops, [a, b], vol, P, O, 24, "gauss", (0, 1, 4, 5))
    for k, net in enumerate((a, b)):
        alone, _, _ = E.stitched_window_logits(ops, [net], vol, P, O, 24, "gauss", (0, 1, 4, 5))
        assert _same_bits(both[k], alone[0]), k
    # the batch size changes no bit either
    other, _, _ = E.stitched_window_logits(ops, [a], vol, P, O, 7, "gauss", (0, 1, 4, 5))
    assert _same_bits(other[0], both[0])


@torch.no_grad()
@pytest.mark.parametrize("flips", [(0, 4), (0, 1, 2, 3), tuple(range(8))])
def test_a_pointwise_net_is_flip_equivariant_so_uniform_tta_changes_nothing(ops, volume, flips):
    vol = volume.to(DEV)
    net = _conv(2, 3, 1, 3).to(DEV)
    base, buf = _parent_path(ops, net, vol, 16)
    got, _, _ = E.stitched_window_logits(ops, [net], vol, P, O, 16, "uniform", flips)
    _, mag, cover = ref_blend([buf.cpu().numpy()], blend_weights_host(P, "uniform"), (N, 3) + VOL, P, O)
    err = np.abs(got[0].cpu().numpy().astype(np.float64) - base.cpu().numpy())
    bound = blend_bound(mag, cover[None, None], len(flips))
    print(f"flips {flips}: max err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()


@torch.no_grad()
@pytest.mark.parametrize("blend", ["gauss", "uniform"])
def test_a_3x3x3_net_against_the_fp64_restatement_of_the_whole_pipeline(ops, volume, blend):
    flips = (0, 1, 2, 3, 4, 5, 6, 7) if blend == "gauss" else (0, 2, 4, 6)
    vol = volume.to(DEV)
    net = _conv(2, 3, 3, 4)
    net64 = _conv(2, 3, 3, 4).double()
    pats = E.image_to_patch3d(volume.double(), P, O)
    passes = []
    for m in flips:
        outs = [_flip(net64(_flip(pt, m, 2)), m, 2) for pt in pats]          # flip, forward, un-flip
        passes.append(torch.cat([v.permute(0, 2, 3, 4, 1) for v in outs]).numpy())
    w = blend_weights_host(P, blend)
    ref, mag, cover = ref_blend(passes, w, (N, 3) + VOL, P, O)
    net = net.to(DEV)
    # the module's own fp32-vs-fp64 difference, on the un-augmented windows
    fwd = net(from_ndhwc(ops.window_gather(vol, P, O))).permute(0, 2, 3, 4, 1).cpu().numpy()
    module_err = float(np.abs(fwd - passes[0]).max())
    margin = blend_bound(mag, cover[None, None], len(flips)) + module_err
    got, _, _ = E.stitched_window_logits(ops, [net], vol, P, O, 16, blend, flips)
    got = got[0].cpu().numpy()
    err = np.abs(got - ref)
    print(f"{blend} {flips}: module err {module_err:.3e}, max err/margin {np.max(err / margin):.3f}")
    assert (err <= margin).all()
    # the zero padding at the window borders is not mirror-symmetric for an asymmetric kernel: the passes show
    plain, _, _ = E.stitched_window_logits(ops, [net], vol, P, O, 16)
    assert (np.abs(got - plain[0].cpu().numpy()) > margin).any()
    # and un-mirroring each pass is what ref_unflip states
    assert np.array_equal(ref_unflip(ref_unflip(passes[1], flips[1]), flips[1]), passes[1])


@torch.no_grad()
def test_validate_seg_tallies_the_blended_logits(ops, volume):
    net = _conv(2, 3, 3, 5).to(DEV)
    lab = torch.randint(0, 3, (N,) + VOL, generator=torch.Generator().manual_seed(9))
    res = E.validate_seg(net, [(volume, lab)], "lits", P, O, window_batch=16, blend="gauss", flips=(0, 4))
    logits, _, _ = E.stitched_window_logits(ops, [net], volume.to(DEV), P, O, 16, "gauss", (0, 4))
    plain, _, _ = E.stitched_window_logits(ops, [net], volume.to(DEV), P, O, 16)
    assert len(res) == N
    for n in range(N):
        want = ops.seg_tallies(logits[0][n], lab[n].to(DEV).to(torch.uint8), "lits", None).cpu()
        assert torch.equal(res[n]["counts"], want) and int(want[0].sum()) == VOL[0] * VOL[1] * VOL[2]
    moved = [ops.seg_tallies(plain[0][n], lab[n].to(DEV).to(torch.uint8), "lits", None).cpu() for n in range(N)]
    assert any(not torch.equal(m, res[n]["counts"]) for n, m in enumerate(moved))       # the switches reached the stitch
    # with the FP network both get the same treatment
    fp = _conv(2, 3, 3, 6).to(DEV)
    res = E.validate_seg(net, [(volume, lab)], "lits", P, O, window_batch=16, fp_model=fp, blend="gauss", flips=(0, 4))
    fl, _, _ = E.stitched_window_logits(ops, [fp], volume.to(DEV), P, O, 16, "gauss", (0, 4))
    counts, _, _, _ = ops.seg_agreement(logits[0][0], fl[0][0], "lits", None, False)
    assert torch.equal(res[0]["vs_fp"]["counts"], counts.cpu())


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_host_side_errors_and_launch_nothing(ops):
    vol = torch.zeros(1, 1, *P, device=DEV)
    win = torch.zeros(1, *P, 3, device=DEV)
    wts = ops.blend_weights(P, "gauss")
    for flip in (8, -1, 1.5, True):
        with pytest.raises(_lib.EffqError, match="flip"):
            ops.window_gather(vol, P, O, flip=flip)
        with pytest.raises(_lib.EffqError, match="flip"):
            ops.window_put(torch.zeros(1, 3, *P, device=DEV), win, flip, False)
    with pytest.raises(_lib.EffqError, match="9 channels"):
        ops.window_put(torch.zeros(1, 9, *P, device=DEV), torch.zeros(1, *P, 9, device=DEV), 0, False)
    with pytest.raises(_lib.EffqError, match="9 channels"):
        ops.window_stitch(torch.zeros(1, *P, 9, device=DEV), (1, 9) + P, P, O, wts, 1)
    with pytest.raises(_lib.EffqError, match="nflip"):
        ops.window_stitch(win, (1, 3) + P, P, O, wts, 0)
    with pytest.raises(_lib.EffqError, match="axis h"):
        ops.window_stitch(win, (1, 3) + P, P, O, (wts[0], wts[1][:-1], wts[2]), 1)
    with pytest.raises(_lib.EffqError, match="weight tensors"):
        ops.window_stitch(win, (1, 3) + P, P, O, wts[:2], 1)
    with pytest.raises(_lib.EffqError, match="buffer slice"):
        ops.window_put(torch.zeros(1, 3, *P, device=DEV), torch.zeros(2, *P, 3, device=DEV), 0, False)
    with pytest.raises(_lib.EffqError, match="contiguous"):
        ops.window_put(torch.zeros(1, 3, *P, device=DEV), torch.zeros(1, 3, *P, device=DEV).permute(0, 2, 3, 4, 1), 0, False)
    # the library itself: EFFQ_ERR_ARG, and the destination is untouched
    ptr = lambda t: t.data_ptr()
    src = torch.ones(1, 3, *P, device=DEV)
    dst = torch.full((1, *P, 3), 7.0, device=DEV)
    out = torch.full((1, 3) + P, 7.0, device=DEV)
    lib, st = ops.lib, ops.stream
    bad = next(k for k, v in _lib._ERR_NAMES.items() if v == "EFFQ_ERR_ARG")
    assert lib.effq_window_put(ptr(src), 1, 3, *P, 8, 0, ptr(dst), st) == bad
    assert lib.effq_window_put(ptr(src), 1, 3, *P, 0, 2, ptr(dst), st) == bad
    assert lib.effq_window_put(ptr(src), 1, 9, *P, 0, 0, ptr(dst), st) == bad
    assert lib.effq_window_put(ptr(src), 1 << 20, 8, 128, 128, 128, 0, 0, ptr(dst), st) == bad        # 2^44 elements
    assert lib.effq_window_gather(ptr(src), 1, 3, *P, *P, *O, 0, 1, 8, ptr(dst), st) == bad
    assert lib.effq_window_gather(ptr(src), 1, 3, *P, *P, *O, 0, 2, 0, ptr(dst), st) == bad           # one window only
    w3 = [ptr(t) for t in wts]
    assert lib.effq_window_stitch(ptr(dst), 1, 3, *P, *P, *O, *w3, 0, ptr(out), st) == bad
    assert lib.effq_window_stitch(ptr(dst), 1, 9, *P, *P, *O, *w3, 1, ptr(out), st) == bad
    assert lib.effq_window_stitch(ptr(dst), 1, 3, *P, *P, *O, w3[0], None, w3[2], 1, ptr(out), st) == bad
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()) and bool((out == 7.0).all())
