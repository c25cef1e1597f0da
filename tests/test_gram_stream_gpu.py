"""The streamed gather of effq_gram_accum (csrc/gram.hip, k_gram_stream) and the k_gram_finish that keeps 16 slab loads in
flight, against the kernels of the previous commits, a numpy restatement of the finish, and fp64 (-m gpu).

Where C1 % 4 == 0 and x sits on the 16-byte grid (effq_gram_streamed), effq_gram_accum reads x by 16-byte cells whose voxel
coordinates are carried from chunk to chunk by addition, reads y by 16-byte cells or (C2 % 4 != 0, y off the grid) by
values, and computes and stores only the 32 x 32 sub-tiles the finish reads.  Every output element still sees the same
MFMA steps in the same order, so:
  * A0 / B0 of aligned inputs (streamed) equal, bit for bit, A0 / B0 of the same values placed 4 bytes past a 16-byte
    boundary (k_gram<true> / k_gram<false>, the kernels of the previous commits), and with x aligned and y off the grid
    (streamed, y by values) where C2 <= 32;
  * A0 / B0 equal a numpy restatement of k_gram_finish on the slabs left in the workspace: sequential fp64 sum in split
    order, float32(2 s), optional fp32 accumulate - for 1, 16, 17 and 35 splits (none, exactly one, one and a tail, two
    and a tail of the groups of 16 loads);
  * a workspace filled with NaN before the call changes nothing (what is no longer written is never read);
  * max |A0 - want| <= 3e-6 max |want| against the fp64 slab reference, the bound of
    tests/test_gram_shapes_gpu.py::test_fp32_gram_in_every_dispatch_class.
Inputs are seeded, carry negative values, exact zeros and an attention map of three distinct weights."""
import numpy as np
import pytest
import torch

from tests.test_gram_shapes_gpu import gram_reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MB = 128


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_ops(DEV)


def _t3(v):
    return (v, v, v) if isinstance(v, int) else tuple(int(i) for i in v)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _off_grid(t):
    """The same values in a buffer that starts 4 bytes past a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert t.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _inputs(shape, geom, c2, seed, with_att):
    """Seeded CPU inputs (NDHWC): signed values, about one exact zero in eight, three attention weights."""
    gen = torch.Generator().manual_seed(seed)
    N, c1, D, H, W = shape
    od, oh, ow = geom.out_dims()
    x = torch.randn(N, D, H, W, c1, generator=gen)
    x[torch.rand(x.shape, generator=gen) < 0.125] = 0.0
    y = torch.randn(N, od, oh, ow, c2, generator=gen)
    y[torch.rand(y.shape, generator=gen) < 0.125] = 0.0
    att = None
    if with_att:
        att = torch.tensor([0.5, 1.0, 2.75])[torch.randint(0, 3, (N, od, oh, ow), generator=gen)]
    return x, y, att


def _check_fp64(A0, B0, x, y, att, k, s, p, bias):
    """The bound of test_fp32_gram_in_every_dispatch_class: 3e-6 of the largest entry, A0 and B0 each."""
    ref = gram_reference(x, y, att, k, s, p, bias, device=DEV)
    wantA, wantB = 2 * ref["A"], 2 * ref["B"]
    ra = float(((A0.double() - wantA).abs().max() / (3e-6 * wantA.abs().max())).item())
    rb = float(((B0.double() - wantB).abs().max() / (3e-6 * wantB.abs().max())).item())
    print(f"   error / bound vs fp64: A0 {ra:.4g}, B0 {rb:.4g}")
    assert ra <= 1.0 and rb <= 1.0, (ra, rb)


# tag, (N, C1, D, H, W), c2, k, stride, pad, bias, attention, expected (NB, vec, fold), y by values when only y is off grid
CASES = [
    ("first-conv", (2, 4, 10, 9, 11), 32, 3, 2, 1, True, True, (2, True, 1)),         # 2 x 150 voxels, E = 141
    ("first-conv-noatt", (2, 4, 10, 9, 11), 32, 3, 2, 1, True, False, (2, True, 1)),
    ("classifier", (2, 32, 7, 6, 5), 3, 1, 1, 0, True, True, (1, False, 1)),           # E = 36, y by values
    ("nobias-8-4", (2, 8, 6, 7, 5), 4, 3, 1, 1, False, True, (2, True, 1)),            # E = 220
    ("two-block-rows", (1, 4, 9, 8, 7), 32, 3, 1, 1, True, True, (2, True, 1)),        # E = 141: 13 rows in block 1
    ("wide-8-8", (2, 8, 6, 7, 5), 8, 3, 1, 1, True, True, (2, True, 1)),               # E = 225
    ("one-block-117", (2, 4, 7, 6, 5), 8, 3, 1, 1, True, True, (1, True, 1)),          # E = 117: 10 sub-tiles, 8 waves
    ("fold4-splits", (1, 4, 104, 101, 100), 3, 1, 1, 0, True, True, (1, False, 4)),    # V = 1 050 400 >= 2^20
]


@pytest.mark.parametrize("tag,shape,c2,k,s,p,bias,with_att,cls", CASES, ids=[c[0] for c in CASES])
def test_streamed_gather_gives_the_plain_kernels_bits(ops, tag, shape, c2, k, s, p, bias, with_att, cls):
    from efficientq_amd.hip_ops import make_geom
    geom = make_geom(shape, c2, k, s, p)
    N, c1, D, H, W = shape
    od, oh, ow = geom.out_dims()
    V = N * od * oh * ow
    E = c1 * int(np.prod(_t3(k))) + c2 + int(bias)
    plan = ops.gram_plan(geom, bias)
    assert (plan["NB"], plan["vec"], plan["fold"]) == cls and plan["NB"] == -(-E // MB), (plan, E)
    if tag.startswith("first-conv"):
        # no multiple of the chunk, a chunk across the two volumes, a partial last chunk
        assert E == 141 and V % 32 != 0 and (od * oh * ow) % 32 != 0, (E, V)
    if tag == "classifier":
        assert E == 36
    if tag == "two-block-rows":
        assert E == 141
    if tag == "wide-8-8":
        assert E == 225
    if tag == "fold4-splits":
        chunks, cps = -(-V // 32), plan["vox_per_split"] // 32
        assert V >= 2 ** 20 and plan["nsplit"] > 16 and cps % 4 != 0, plan
    x, y, att = _inputs(shape, geom, c2, 4000 + len(tag) + c2, with_att)
    xd, yd = x.to(DEV), y.to(DEV)
    ad = None if att is None else att.to(DEV)
    xo, yo = _off_grid(xd), _off_grid(yd)
    assert ops.gram_streamed(xd, yd, geom, bias) and not ops.gram_streamed(xo, yo, geom, bias)
    assert ops.gram_streamed(xd, yo, geom, bias) == (c2 <= 32)           # y by values whatever C2 % 4 is
    A0, B0 = ops.gram(xd, ad, yd, geom, bias)
    A1, B1 = ops.gram(xo, ad, yo, geom, bias)
    A2, B2 = ops.gram(xd, ad, yo, geom, bias)
    torch.cuda.synchronize()
    assert torch.isfinite(A0).all() and torch.isfinite(B0).all()
    assert _same_bits(A0, A1) and _same_bits(B0, B1), "the streamed gather and the plain kernel differ"
    assert _same_bits(A0, A2) and _same_bits(B0, B2), "y by values and y by cells differ"
    assert torch.equal(A0, A0.T)
    # what is no longer written is never read
    ws = ops._ws["gram"]
    ws[:ws.numel() // 8 * 8].view(torch.float64).fill_(float("nan"))
    A3, B3 = ops.gram(xd, ad, yd, geom, bias)
    torch.cuda.synchronize()
    assert torch.isfinite(A3).all() and torch.isfinite(B3).all()
    assert _same_bits(A0, A3) and _same_bits(B0, B3), "results depend on the workspace's content"
    _check_fp64(A0, B0, x, y, att, k, s, p, bias)


def test_three_input_channels_stay_on_the_plain_kernel(ops):
    from efficientq_amd.hip_ops import make_geom
    shape, c2, k = (2, 3, 7, 6, 5), 8, 3
    geom = make_geom(shape, c2, k, 1, 1)
    x, y, att = _inputs(shape, geom, c2, 4100, True)
    xd, yd, ad = x.to(DEV), y.to(DEV), att.to(DEV)
    assert xd.data_ptr() % 16 == 0 and yd.data_ptr() % 16 == 0
    assert not ops.gram_streamed(xd, yd, geom, True) and not ops.gram_plan(geom, True)["vec"]
    A0, B0 = ops.gram(xd, ad, yd, geom, True)
    torch.cuda.synchronize()
    _check_fp64(A0, B0, x, y, att, k, 1, 1, True)


def _restate_finish(slabs, geom, bias, plan, prior=None):
    """k_gram_finish in numpy on slabs [nsplit, npairs, 128, 128] (float64): reference row c * T + tap <-> tap-major row
    tap * C1 + c, bias row RX + C2, the pair (ri <= rj) of block pair (I, J), sequential sum in split order."""
    c1, c2 = geom.C1, geom.C2
    T = geom.KD * geom.KH * geom.KW
    RX = T * c1
    n = RX + int(bias)
    NB = plan["NB"]
    q = np.arange(n)
    to_int = (q % T) * c1 + q // T
    if bias:
        to_int[n - 1] = RX + c2

    def total(ri, rj):
        lo, hi = np.minimum(ri, rj), np.maximum(ri, rj)
        I, J = lo // MB, hi // MB
        pidx = I * NB - I * (I - 1) // 2 + (J - I)
        s = np.zeros(lo.shape, dtype=np.float64)
        for kk in range(slabs.shape[0]):                     # one addition per split, in split order
            s = s + slabs[kk][pidx, lo - I * MB, hi - J * MB]
        return (2.0 * s).astype(np.float32)

    A = total(to_int[:, None] + 0 * to_int[None, :], to_int[None, :] + 0 * to_int[:, None])
    B = total(to_int[None, :] + np.zeros((c2, 1), dtype=np.int64), (RX + np.arange(c2))[:, None] + 0 * to_int[None, :])
    if prior is not None:
        A, B = prior[0] + A, prior[1] + B                    # float32 + float32
    return A, B


# tag, (N, C1, D, H, W), c2, k, pad, nsplit
FINISH_CASES = [
    ("1-split", (1, 8, 4, 4, 4), 3, 1, 0, 1),
    ("16-splits", (1, 8, 16, 16, 16), 3, 1, 0, 16),
    ("17-splits-two-blocks", (1, 4, 16, 16, 17), 32, 3, 1, 17),
    ("35-splits", (1, 8, 16, 16, 35), 3, 1, 0, 35),
]


@pytest.mark.parametrize("tag,shape,c2,k,p,nsplit", FINISH_CASES, ids=[c[0] for c in FINISH_CASES])
def test_finish_against_a_restatement(ops, tag, shape, c2, k, p, nsplit):
    import ctypes as C
    from efficientq_amd.hip_ops import make_geom
    geom = make_geom(shape, c2, k, 1, p)
    plan = ops.gram_plan(geom, True)
    assert plan["nsplit"] == nsplit, plan
    x, y, att = _inputs(shape, geom, c2, 4200 + nsplit, True)
    xd, yd, ad = x.to(DEV), y.to(DEV), att.to(DEV)
    assert ops.gram_streamed(xd, yd, geom, True)
    A0, B0 = ops.gram(xd, ad, yd, geom, True)
    torch.cuda.synchronize()
    nslab = plan["nsplit"] * plan["npairs"] * MB * MB
    assert ops.lib.effq_gram_ws_bytes(C.byref(geom), 1) >= 8 * nslab
    slabs = ops._ws["gram"][:8 * nslab].view(torch.float64).cpu().numpy().reshape(plan["nsplit"], plan["npairs"], MB, MB)
    wantA, wantB = _restate_finish(slabs, geom, True, plan)
    assert np.array_equal(A0.cpu().numpy().view(np.int32), wantA.view(np.int32))
    assert np.array_equal(B0.cpu().numpy().view(np.int32), wantB.view(np.int32))
    # accumulate: a second call into the same A0 / B0 adds the same values in fp32
    A1, B1 = ops.gram(xd, ad, yd, geom, True, A0.clone(), B0.clone())
    torch.cuda.synchronize()
    accA, accB = _restate_finish(slabs, geom, True, plan, prior=(wantA, wantB))
    assert np.array_equal(A1.cpu().numpy().view(np.int32), accA.view(np.int32))
    assert np.array_equal(B1.cpu().numpy().view(np.int32), accB.view(np.int32))
