"""The pipelined gather of effq_gram_f64 (csrc/gram_f64.hip, k_gram_f64<TPW, true>) against its plain loop and fp64 (-m gpu).

effq_gram_f64 reads x by 16-byte cells, prefetches the cells of the next chunk into registers and carries every cell's
output-voxel coordinates from chunk to chunk by a mixed-radix addition where the layer allows it (effq_gram_f64_pipelined);
everywhere else it runs the plain loop.  Both stage the same LDS rows, so on every case:
  * Au / Bu of 16-byte aligned inputs (pipelined) equal, bit for bit, Au / Bu of the same values placed 4 bytes past a
    16-byte boundary (plain loop) - the plain loop is the kernel of the previous commits;
  * every entry obeys the summation bound 2 (V - 1) 2^-53 sum_v |x_i(v) x_j(v)| against an fp64 im2col product on the CPU
    (products of fp32 values are exact in fp64, so every summation order obeys (V - 1) 2^-53 sum |.|; both sides carry it);
  * Au is symmetric, nothing depends on the workspace's content.
Cases: the first-conv class (4 -> 8 and 4 -> 32, 3^3: 11 tiles per wave, four cells of x per thread, the last one on 96
threads only; 32 targets = exactly one cell of y per thread), with and without bias; the classifier class (32 -> 3, 1^3:
3 tiles per wave, one cell of x, y by values); 8 -> 8 at 1 x 3 x 3 (6 tiles per wave); and, where the carried coordinates
and the prefetch under the matrix-core loop do their work, launches whose 1024 persistent workgroups walk 2 - 3 chunks over
2 or 3 volumes, stride 2 included, the last chunk short.  Geometries outside the pipelined form (C1 = 1; 40 targets) are
asserted to stay on the plain loop."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_ops(DEV)


def _t3(v):
    return (v, v, v) if isinstance(v, int) else tuple(int(i) for i in v)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _patches(x, k, s, p, bias):
    """V x n fp64 patch matrix of x [N, D, H, W, C1]: rows in voxel order, columns (c1, kd, kh, kw) then the ones entry."""
    xp = F.pad(x.double(), (0, 0, p[2], p[2], p[1], p[1], p[0], p[0]))
    win = xp.unfold(1, k[0], s[0]).unfold(2, k[1], s[1]).unfold(3, k[2], s[2])       # N, OD, OH, OW, C1, kd, kh, kw
    P = win.reshape(-1, x.shape[-1] * k[0] * k[1] * k[2])
    if bias:
        P = torch.cat([P, torch.ones(P.shape[0], 1, dtype=torch.float64)], 1)
    return P


def _off_grid(t):
    """The same values in a buffer that starts 4 bytes past a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert t.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


# tag, (N, C1, D, H, W), c2, k, stride, pad, bias, tiles per wave, walks several chunks
CASES = [
    ("first-conv", (2, 4, 11, 9, 13), 8, 3, 2, 1, True, 11, False),              # 420 voxels: 13 chunks and 4 voxels
    ("first-conv-nobias", (2, 4, 11, 9, 13), 8, 3, 2, 1, False, 11, False),
    ("first-conv-32-targets", (1, 4, 9, 8, 7), 32, 3, 1, 1, True, 11, False),    # 256 cells of y: one per thread
    ("classifier", (2, 32, 5, 6, 7), 3, 1, 1, 0, True, 3, False),
    ("8-to-8-k133", (2, 8, 5, 7, 6), 8, (1, 3, 3), 1, (0, 1, 1), True, 6, False),   # n = 73, 20 tiles
    ("first-conv-walk", (3, 4, 60, 61, 65), 32, 3, 2, 1, True, 11, True),        # 3 x 30 690 voxels: 2878 chunks
    ("classifier-walk", (2, 32, 30, 31, 37), 3, 1, 1, 0, True, 3, True),         # 2 x 34 410 voxels: 2151 chunks
    ("8-to-8-k133-walk", (2, 8, 30, 31, 37), 8, (1, 3, 3), 1, (0, 1, 1), True, 6, True),
]


@pytest.mark.parametrize("tag,shape,c2,k,s,p,bias,tpw,walk", CASES, ids=[c[0] for c in CASES])
def test_pipelined_gather_gives_the_plain_loops_bits(ops, tag, shape, c2, k, s, p, bias, tpw, walk):
    from efficientq_amd.hip_ops import make_geom
    geom = make_geom(shape, c2, k, s, p)
    k, s, p = _t3(k), _t3(s), _t3(p)
    N, c1, D, H, W = shape
    od, oh, ow = geom.out_dims()
    V = N * od * oh * ow
    plan = ops.gram_f64_plan(geom, bias)
    assert plan["tpw"] == tpw, plan
    if walk:
        assert plan["grid"] == 1024 and plan["nchunk"] > 2 * plan["grid"] and plan["nchunk"] % plan["grid"] != 0, plan
        assert V % 32 != 0 and (od * oh * ow) % 32 != 0          # a short last chunk, chunks across volume boundaries
    gen = torch.Generator().manual_seed(17 + len(tag))
    x = torch.randn(N, D, H, W, c1, generator=gen)
    y = torch.randn(N, od, oh, ow, c2, generator=gen)
    P = _patches(x, k, s, p, bias)
    Y = y.double().reshape(V, c2)
    refA, refB = P.T @ P, Y.T @ P
    absA, absB = P.abs().T @ P.abs(), Y.abs().T @ P.abs()

    xd, yd = x.to(DEV), y.to(DEV)
    xo, yo = _off_grid(xd), _off_grid(yd)
    assert ops.gram_f64_pipelined(xd, yd, geom, bias) and not ops.gram_f64_pipelined(xo, yo, geom, bias)
    Au, Bu = ops.gram_f64(xd, yd, geom, bias)
    Au1, Bu1 = ops.gram_f64(xo, yo, geom, bias)
    if walk:                                                     # the library zero-fills a workspace only when it allocates it
        ops._ws["gram_f64"].fill_(0xFF)
    Au2, Bu2 = ops.gram_f64(xd, yd, geom, bias)
    torch.cuda.synchronize()
    assert _same_bits(Au, Au1) and _same_bits(Bu, Bu1), "the pipelined gather and the plain loop differ"
    assert _same_bits(Au, Au2) and _same_bits(Bu, Bu2), "results depend on the call or on the workspace's content"
    assert torch.equal(Au, Au.T)
    worst = 0.0
    for got, want, ab in ((Au, refA, absA), (Bu, refB, absB)):
        err = (got.cpu() - want).abs()
        bound = 2.0 * max(V - 1, 1) * U53 * ab
        assert bool((err[bound == 0] == 0).all())
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print(f"{tag}: error / bound = {worst:.4g}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("shape,c2,k,why", [((2, 1, 7, 6, 9), 8, 3, "C1 = 1"), ((1, 4, 6, 5, 7), 40, 3, "320 cells of y"),
                                             ((1, 128, 4, 4, 4), 64, 1, "18 tiles per wave")])
def test_other_layers_stay_on_the_plain_loop(ops, shape, c2, k, why):
    from efficientq_amd.hip_ops import make_geom
    geom = make_geom(shape, c2, k, 1, k // 2)
    assert ops.gram_f64_supported(geom, False)
    N, c1, D, H, W = shape
    x = torch.zeros(N, D, H, W, c1, device=DEV)
    od, oh, ow = geom.out_dims()
    y = torch.zeros(N, od, oh, ow, c2, device=DEV)
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    assert not ops.gram_f64_pipelined(x, y, geom, False), why
