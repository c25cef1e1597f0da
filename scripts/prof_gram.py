"""Time effq_gram_accum on the first conv / classifier shapes of the BraTS net (16 volumes): the streamed gather (inputs
on the 16-byte grid) against the plain kernels (the same values 4 bytes off it), and k_gram_finish alone on the slabs of
the last call.  `python scripts/prof_gram.py wide` times the dominant quantised-layer shape (32 ch, 3^3, 16 x 64^3) too."""
import ctypes as C
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from efficientq_amd._lib import check
from efficientq_amd.hip_ops import get_ops, make_geom, _ptr
dev = "cuda:0"; ops = get_ops(dev)


def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


shapes = [(4, 32, 3, 2, 1, 128), (32, 3, 1, 1, 0, 64)]
if "wide" in sys.argv[1:]:
    shapes.append((32, 32, 3, 1, 1, 64))
for (c1, c2, k, s, p, S) in shapes:
    N = 16
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, S, S, S, c1, generator=g).to(dev)
    geom = make_geom((N, c1, S, S, S), c2, k, s, p)
    od, oh, ow = geom.out_dims()
    y = torch.randn(N, od, oh, ow, c2, generator=g).to(dev)
    att = torch.randint(1, 3, (N, od, oh, ow), generator=g).float().to(dev)
    n = c1 * k ** 3 + 1; V = N * od * oh * ow
    fl = 2.0 * n * n * V + 2.0 * c2 * n * V
    xb, yb = torch.zeros(x.numel() + 1, device=dev), torch.zeros(y.numel() + 1, device=dev)
    xo, yo = xb[1:].view(x.shape).copy_(x), yb[1:].view(y.shape).copy_(y)
    plan = ops.gram_plan(geom, True)
    out = {}
    for tag, a, b in (("streamed", x, y), ("plain", xo, yo)):
        assert ops.gram_streamed(a, b, geom, True) == (tag == "streamed")
        ms = timed(lambda: ops.gram(a, att, b, geom, True))
        out[tag] = ops.gram(a, att, b, geom, True)
        print(f"gram {c1}->{c2} k{k} n={n} V={V} {tag}: {ms:.3f} ms (both launches)  {fl / ms / 1e9:.1f} TFLOP/s algorithmic "
              f"({fl / ms / 1e9 / 157.3 * 100:.1f}% of f32 MFMA peak)  {plan}")
    torch.cuda.synchronize()
    same = all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(out["streamed"], out["plain"]))
    A0, B0 = out["streamed"]
    ws = ops._ws["gram"]
    ms = timed(lambda: check(ops.lib.effq_gram_finish(C.byref(geom), 1, _ptr(A0), _ptr(B0), 0, _ptr(ws), ws.numel(),
                                                      ops.stream), "effq_gram_finish"))
    print(f"gram {c1}->{c2} k{k} k_gram_finish alone ({plan['nsplit']} splits): {ms:.3f} ms; streamed == plain bit for bit: {same}")
