"""Every dispatch class of the Gram kernels (csrc/gram.hip, gram_i8.hip, gram_f64.hip, gram_loss.hip, gram_loss_i8.hip)
against fp64 (-m gpu).

The Gram system (A0, B0 and the unweighted Au, Bu the per-iteration losses are formed from) feeds every other stage of a
calibration.  Each case here first asserts, through effq_gram_plan_query / effq_gram_i8_plan_query /
effq_gram_f64_plan_query, the class it was chosen for - a retuned threshold then fails the case instead of silently moving
it to a class that is tested elsewhere - and then compares the kernels with fp64 arithmetic on the same inputs:

  a. effq_gram_f64: persistent workgroups that walk 2, 3 and 3-or-4 chunks, every instantiation (3, 6, 11, 18 tiles per
     wave), n = 128 exactly with and without the bias row and 68 tiles, strides (2, 2, 1) without padding, chunks that
     straddle a volume boundary.  Bound, entry by entry: |err_ij| <= (V - 1) 2^-53 sum_v |x_i(v) x_j(v)| (the products of
     fp32 values are exact in fp64, so every summation order obeys it) against a np.longdouble sum where V is small, twice
     that against the fp64 slab reference elsewhere;
  b. effq_gram_accum: fold = 4 (from 2^20 voxels) with a tail that is not a multiple of the fold, on both k_gram
     instantiations; k_gram<false> on two macro blocks; the strided k_gram_finish at n = 1729 and 3457, accumulate = 1 on
     top of a prior result; E = 125, 127, 128, 129 rows; one split, and a last split of one chunk.  Bound: 3e-6 max |A0|;
  c. effq_gram_accum_i8 / _unw: a 32 -> 32 layer at 2^20 voxels (94 chunks per split, 88 splits) at 4 and 16 levels, without
     and with a voxel list; 128 levels with every id at 127; 16 classes on a multi-block system with a class of 5 voxels,
     classes of exactly 128 and 256, weights present in the first volume only, and a hand-made list with an empty class.
     The unweighted integer system is compared for EQUALITY after the documented scaling;
  d. effq_gram_loss at n = 3457 and 6913 and a c2 that is not a multiple of 32; effq_gram_loss_i8 with 1, 4, 5 and 6 digit
     planes at the capacity of each plane count and one above it, count = 1 and 16, one partial column tile, nw = 64 and
     6912, three groups on one workspace, and the error flag of effq_gram_loss_i8_prepare.

Classes that no sane size reaches: the 65 535 clamp on the splits of effq_gram_accum needs 65 535 * 8 chunks of 32 voxels
with one block pair AND 4096 / npairs >= 65 535, which no system has (npairs >= 1 caps the wish at 4096 splits);
GI_MAX_CPS = 1000 chunks per split of effq_gram_accum_i8 needs more than 3072 * 1000 * 128 = 3.9e8 voxels on a one-block
system (tests/test_host_cpu.py asserts through the query that the clamp keeps the int32 partial sums in range).

Outputs of (a) and (b) land in NaN-filled blocks between guard bands, and every case of (a) - (c) runs a second time on a
workspace filled with 0xFF bytes: the library zero-fills a workspace only when it allocates it.  The references are an
im2col by strided views multiplied slab by slab in fp64 (gram_reference; tests/test_host_cpu.py ties it to the oracle's
patch_matrix / ProxSystem) - on the device for the large cases, a different code path from every kernel under test."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                     # elements on either side of an output
SENTINEL = -7.25e33
SLAB = 65536                   # output voxels per slab of the reference
U53 = 2.0 ** -53
_worst = {}


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_ops(DEV)


def dev(t):
    return None if t is None else t.to(DEV)


def _t3(v):
    return (v, v, v) if isinstance(v, int) else tuple(int(i) for i in v)


def _record(group, tag, ratio):
    _worst.setdefault(group, {})[tag] = float(ratio)
    print(f"{group} {tag}: error / bound = {ratio:.4g} (worst of the group so far {max(_worst[group].values()):.4g})")


def _guarded(shape, dtype=torch.float32):
    """A NaN-filled device tensor of `shape` inside a larger sentinel-filled buffer: (buffer, view)."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + numel].view(*shape)
    view.fill_(float("nan"))
    return buf, view


def _guards_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all().item()) and bool((buf[-GUARD:] == SENTINEL).all().item())


def _same_bits(a, b):
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ------------------------------------------------------------------ the reference
def gram_reference(x, y, att, k, s, p, bias, device="cpu", G=None, b=None, want_abs=False, want_patches=False, slab=SLAB):
    """The Gram sums of one layer in fp64: x [N, D, H, W, C1], y [N, OD, OH, OW, C2], att [N, OD, OH, OW] or None.
    The im2col is a strided window view of the zero-padded input (rows in the reference's (c1, kd, kh, kw) order, then the
    ones entry of the bias), taken one slab of output voxels at a time:
      A = sum_v a_v xhat xhat^T, B = sum_v a_v y xhat^T (no factor 2), Au / Bu the same without a_v,
      absA / absB = sum_v |xhat_i xhat_j|, sum_v |y_c xhat_j| (want_abs), loss = sum (xhat . [G | b] - y)^2 (G given),
      patches = the whole V x n matrix (want_patches; small cases only)."""
    k, s, p = _t3(k), _t3(s), _t3(p)
    x64, y64 = x.to(device).double(), y.to(device).double()
    a64 = None if att is None else att.to(device).double()
    N, c1, c2 = int(x64.shape[0]), int(x64.shape[-1]), int(y64.shape[-1])
    xp = F.pad(x64, (0, 0, p[2], p[2], p[1], p[1], p[0], p[0]))
    win = xp.unfold(1, k[0], s[0]).unfold(2, k[1], s[1]).unfold(3, k[2], s[2])       # N, OD, OH, OW, C1, kd, kh, kw
    od, oh, ow = (int(i) for i in win.shape[1:4])
    assert tuple(y64.shape) == (N, od, oh, ow, c2), (tuple(y64.shape), (N, od, oh, ow, c2))
    nw = c1 * k[0] * k[1] * k[2]
    n = nw + int(bias)
    z = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=device)
    out = dict(A=z(n, n), B=z(c2, n), Au=z(n, n), Bu=z(c2, n), V=N * od * oh * ow, n=n)
    if want_abs:
        out.update(absA=z(n, n), absB=z(c2, n))
    Gm = None
    if G is not None:
        Gm = G.to(device).double().reshape(c2, nw)
        if bias:
            Gm = torch.cat([Gm, b.to(device).double().reshape(c2, 1)], 1)
        out["loss"] = 0.0
    rows = []
    step = max(1, slab // (oh * ow))
    for i in range(N):
        for d0 in range(0, od, step):
            d1 = min(od, d0 + step)
            P = win[i, d0:d1].reshape(-1, nw)
            if bias:
                P = torch.cat([P, torch.ones(P.shape[0], 1, dtype=torch.float64, device=device)], 1)
            Y = y64[i, d0:d1].reshape(-1, c2)
            out["Au"] += P.T @ P
            out["Bu"] += Y.T @ P
            if a64 is not None:
                PW = P * a64[i, d0:d1].reshape(-1, 1)
                out["A"] += P.T @ PW
                out["B"] += Y.T @ PW
            if want_abs:
                out["absA"] += P.abs().T @ P.abs()
                out["absB"] += Y.abs().T @ P.abs()
            if Gm is not None:
                out["loss"] += float(((P @ Gm.T - Y) ** 2).sum().item())
            if want_patches:
                rows.append(P.cpu())
    if a64 is None:
        out["A"], out["B"] = out["Au"].clone(), out["Bu"].clone()
    if want_patches:
        out["patches"] = torch.cat(rows)
    return out


def _geom(shape, c2, k, s, p):
    """shape = (N, C1, D, H, W) as make_geom takes it."""
    from efficientq_amd.hip_ops import make_geom
    return make_geom(shape, c2, k, s, p)


def _inputs(shape, geom, c2, seed, relu=True):
    """Seeded CPU inputs in the kernels' NDHWC layout: x, y, and the generator for whatever else the case draws."""
    gen = torch.Generator().manual_seed(seed)
    N, c1, D, H, W = shape
    x = torch.randn(N, D, H, W, c1, generator=gen)
    if relu:
        x = torch.relu(x)
    od, oh, ow = geom.out_dims()
    y = torch.randn(N, od, oh, ow, c2, generator=gen)
    return x, y, gen


# ------------------------------------------------------------------ a. effq_gram_f64
# tag, (N, C1, D, H, W), c2, k, stride, pad, bias, tpw, chunks per workgroup (min, max), longdouble reference
F64_CASES = [
    ("classifier-2chunks", (1, 32, 32, 32, 33), 3, 1, 1, 0, True, 3, (1, 2), False),      # V = 33 792: 32 workgroups walk 2
    ("classifier-3chunks", (3, 32, 32, 32, 32), 3, 1, 1, 0, True, 3, (3, 3), False),      # V = 3 * 32 768
    ("first-conv-ragged", (1, 4, 46, 47, 47), 32, 3, 1, 1, True, 11, (3, 4), False),      # V = 101 614, last chunk short
    ("tpw6-s221-nopad-N3", (3, 2, 60, 60, 41), 16, 3, (2, 2, 1), 0, True, 6, (3, 4), False),   # n = 55, 14 tiles
    ("n128-bias-68tiles", (2, 127, 10, 10, 10), 64, 1, 1, 0, True, 18, (1, 1), True),     # n = GF_MAXN with the ones row
    ("n128-nobias-68tiles", (2, 128, 10, 10, 10), 64, 1, 1, 0, False, 18, (1, 1), True),
    ("n128-bias-68tiles-2chunks", (3, 127, 24, 24, 24), 64, 1, 1, 0, True, 18, (1, 2), False),   # V = 41 472
    ("c2-40-49tiles", (2, 4, 10, 10, 10), 40, 3, 1, 1, True, 18, (1, 1), True),           # C2 in 33..48
    ("first-conv-s221-nopad-N1", (1, 4, 21, 20, 19), 32, 3, (2, 2, 1), 0, True, 11, (1, 1), True),
    ("tpw6-small", (3, 2, 13, 12, 9), 8, 3, (2, 2, 1), 0, False, 6, (1, 1), True),        # n = 54 without bias
]


def _run_gram_f64(ops, x, y, geom, bias, n):
    from efficientq_amd.hip_ops import _ptr
    from efficientq_amd._lib import check
    abuf, Au = _guarded((n, n), torch.float64)
    bbuf, Bu = _guarded((geom.C2, n), torch.float64)
    ws = ops._workspace("gram_f64", ops.lib.effq_gram_f64_ws_bytes(C.byref(geom), int(bias)))
    check(ops.lib.effq_gram_f64(_ptr(x), _ptr(y), C.byref(geom), int(bias), _ptr(Au), _ptr(Bu), _ptr(ws), ws.numel(),
                                ops.stream), "effq_gram_f64")
    torch.cuda.synchronize()
    assert _guards_untouched(abuf) and _guards_untouched(bbuf), "effq_gram_f64 wrote outside Au / Bu"
    return Au, Bu


@pytest.mark.parametrize("tag,shape,c2,k,s,p,bias,tpw,walk,small", F64_CASES, ids=[c[0] for c in F64_CASES])
def test_fp64_gram_in_every_dispatch_class(ops, tag, shape, c2, k, s, p, bias, tpw, walk, small):
    """effq_gram_f64 against the fp64 slab reference (and np.longdouble sums where V is small) within the summation bound
    (V - 1) 2^-53 sum |x_i x_j| per entry; the loss effq_gram_loss forms from the result against the fp64 conv loss at
    1e-10.  Largest error / bound seen on an MI355X: 0.0058 for the system (the bound is a worst case over V additions),
    4e-6 for the loss."""
    geom = _geom(shape, c2, k, s, p)
    assert ops.gram_f64_supported(geom, bias)
    plan = ops.gram_f64_plan(geom, bias)
    od, oh, ow = geom.out_dims()
    V = shape[0] * od * oh * ow
    assert plan["tpw"] == tpw and plan["nchunk"] == -(-V // 32) and plan["grid"] == min(plan["nchunk"], 1024), plan
    assert (plan["nchunk"] // plan["grid"], -(-plan["nchunk"] // plan["grid"])) == walk, plan
    if tag == "first-conv-ragged":
        assert V % 32 != 0 and plan["nchunk"] % plan["grid"] != 0
    if tag == "tpw6-s221-nopad-N3":
        assert (od * oh * ow) % 32 != 0                      # a chunk straddles the volume boundary
    if "68tiles" in tag:
        assert plan["ntiles"] == 68
    x, y, gen = _inputs(shape, geom, c2, 1000 + len(tag) + c2, relu=False)
    G = torch.randn(c2, shape[1] * int(np.prod(_t3(k))), generator=gen) * 0.1
    b = torch.randn(c2, generator=gen) * 0.1 if bias else None
    ref = gram_reference(x, y, None, k, s, p, bias, device=DEV, G=G, b=b, want_abs=True, want_patches=small)
    n = ref["n"]
    dx, dy = dev(x), dev(y)
    Au, Bu = _run_gram_f64(ops, dx, dy, geom, bias, n)
    assert torch.isfinite(Au).all() and torch.isfinite(Bu).all()
    assert torch.equal(Au, Au.T)
    ratio = 0.0
    if small and np.finfo(np.longdouble).nmant >= 63:
        # 64-bit significands: the reference's own error is 2^-11 of the bound, the differences are taken in longdouble too
        Xl = ref["patches"].numpy().astype(np.longdouble)
        Yl = y.reshape(-1, c2).numpy().astype(np.longdouble)
        for got, want, ab in ((Au, Xl.T @ Xl, ref["absA"]), (Bu, Yl.T @ Xl, ref["absB"])):
            err = np.abs(got.cpu().numpy().astype(np.longdouble) - want)
            bound = ((V - 1) * U53 * ab.cpu().numpy()).astype(np.longdouble)
            assert (err[bound == 0] == 0).all()
            ratio = max(ratio, float((err / np.maximum(bound, 1e-300)).max()))
    else:
        for got, want, ab in ((Au, ref["Au"], ref["absA"]), (Bu, ref["Bu"], ref["absB"])):
            err = (got - want).abs()
            bound = 2.0 * (V - 1) * U53 * ab                  # against another fp64 sum: both carry the bound
            assert bool((err[bound == 0] == 0).all())
            ratio = max(ratio, float((err / bound.clamp_min(1e-300)).max().item()))
    _record("a.gram_f64", tag, ratio)
    assert ratio <= 1.0, ratio
    # repeat call, then on a workspace of 0xFF bytes: the slabs are fully overwritten or they are not
    Au2, Bu2 = _run_gram_f64(ops, dx, dy, geom, bias, n)
    assert _same_bits(Au, Au2) and _same_bits(Bu, Bu2)
    ops._ws["gram_f64"].fill_(0xFF)
    Au3, Bu3 = _run_gram_f64(ops, dx, dy, geom, bias, n)
    assert _same_bits(Au, Au3) and _same_bits(Bu, Bu3)
    # the loss of an iterate from the result
    syy = (dy.double() ** 2).sum().reshape(1)
    got = ops.gram_loss(Au.contiguous(), Bu.contiguous(), syy, dev(G), dev(b)).cpu().tolist()
    _record("a.gram_f64 loss", tag, abs(got[0] - ref["loss"]) / (1e-10 * ref["loss"]))
    assert abs(got[0] - ref["loss"]) <= 1e-10 * ref["loss"], (got, ref["loss"])


# ------------------------------------------------------------------ b. effq_gram_accum
# tag, (N, C1, D, H, W), c2, k, stride, pad, bias, with attention weights
GRAM_CASES = [
    ("fold4-vec", (1, 4, 102, 102, 101), 32, 3, 1, 1, True, True),            # V = 1 050 804, 25 chunks per split
    ("fold4-rows", (1, 3, 104, 101, 101), 5, 1, 1, 0, True, True),            # k_gram<false> at fold 4
    ("rows-two-blocks-6-2", (2, 6, 9, 10, 11), 2, 3, 1, 1, True, True),       # E = 165: x | y inside a cell of block 1
    ("rows-two-blocks-3-5", (2, 3, 9, 10, 11), 5, (5, 3, 3), 1, (2, 1, 1), True, True),   # E = 141: a cell across taps at row 128
    ("finish-strided-1729", (1, 64, 12, 13, 14), 64, 3, 1, 1, True, True),
    ("finish-strided-3457", (1, 128, 12, 13, 14), 128, 3, 1, 1, True, False),
    ("E125", (2, 4, 7, 6, 5), 16, 3, 1, 1, True, True),                       # last block ends in padding rows
    ("E127-rows", (2, 4, 7, 6, 5), 18, 3, 1, 1, True, True),
    ("E128", (2, 4, 7, 6, 5), 20, 3, 1, 1, False, True),                      # last block full
    ("E129", (2, 4, 7, 6, 5), 20, 3, 1, 1, True, False),                      # block 1 holds the ones row alone
    ("one-split", (1, 4, 6, 8, 9), 8, 3, 1, 1, True, True),                   # 14 chunks
    ("last-split-one-chunk", (1, 4, 8, 17, 17), 8, 3, 1, 1, True, True),      # 73 chunks in 9 splits of 9
]


def _run_gram(ops, x, att, y, geom, bias, n, prior=None):
    from efficientq_amd.hip_ops import _ptr
    from efficientq_amd._lib import check
    abuf, A0 = _guarded((n, n))
    bbuf, B0 = _guarded((geom.C2, n))
    if prior is not None:
        A0.copy_(prior[0])
        B0.copy_(prior[1])
    ws = ops._workspace("gram", ops.lib.effq_gram_ws_bytes(C.byref(geom), int(bias)))
    check(ops.lib.effq_gram_accum(_ptr(x), _ptr(att), _ptr(y), C.byref(geom), int(bias), _ptr(A0), _ptr(B0),
                                  int(prior is not None), _ptr(ws), ws.numel(), ops.stream), "effq_gram_accum")
    torch.cuda.synchronize()
    assert _guards_untouched(abuf) and _guards_untouched(bbuf), "effq_gram_accum wrote outside A0 / B0"
    return A0, B0


@pytest.mark.parametrize("tag,shape,c2,k,s,p,bias,with_att", GRAM_CASES, ids=[c[0] for c in GRAM_CASES])
def test_fp32_gram_in_every_dispatch_class(ops, tag, shape, c2, k, s, p, bias, with_att):
    """effq_gram_accum against the fp64 slab reference: max |A0 - want| <= 3e-6 max |want| and the same for B0 (the bound of
    test_gram_vs_oracle), exact symmetry, bit-identical repeats, also on a 0xFF-filled workspace."""
    geom = _geom(shape, c2, k, s, p)
    plan = ops.gram_plan(geom, bias)
    od, oh, ow = geom.out_dims()
    V = shape[0] * od * oh * ow
    chunks = -(-V // 32)
    cps = plan["vox_per_split"] // 32
    E = shape[1] * int(np.prod(_t3(k))) + c2 + int(bias)
    assert plan["NB"] == -(-E // 128) and plan["npairs"] == plan["NB"] * (plan["NB"] + 1) // 2, plan
    assert plan["vec"] == (shape[1] % 4 == 0 and c2 % 4 == 0), plan
    assert plan["fold"] == (4 if tag.startswith("fold4") else 1), plan
    if tag.startswith("fold4"):
        last = chunks - (plan["nsplit"] - 1) * cps
        assert V >= 2 ** 20 and cps % 4 != 0 and last % 4 != 0 and plan["vec"] == (tag == "fold4-vec"), (plan, last)
    if tag == "fold4-vec":
        assert V % 32 != 0
    if tag.startswith("rows") or tag.endswith("rows"):
        assert not plan["vec"]
    if tag.startswith("rows-two-blocks"):
        assert plan["NB"] == 2
    if tag.startswith("finish-strided"):
        n_ = shape[1] * 27 + 1
        assert plan["finish_blocks"] == 8192 and n_ * n_ + c2 * n_ > 8192 * 256, plan
    else:
        assert plan["finish_blocks"] < 8192, plan
    if tag.startswith("E1"):
        assert E == int(tag[1:4]), E
    if tag == "one-split":
        assert plan["nsplit"] == 1 and chunks < 16, plan
    if tag == "last-split-one-chunk":
        assert plan["nsplit"] > 1 and chunks - (plan["nsplit"] - 1) * cps == 1, plan
    x, y, gen = _inputs(shape, geom, c2, 2000 + len(tag) + c2)
    att = torch.randint(1, 4, (shape[0], od, oh, ow), generator=gen).float() if with_att else None
    ref = gram_reference(x, y, att, k, s, p, bias, device=DEV)
    n = ref["n"]
    wantA, wantB = 2 * ref["A"], 2 * ref["B"]
    dx, dy, da = dev(x), dev(y), dev(att)
    A0, B0 = _run_gram(ops, dx, da, dy, geom, bias, n)
    assert torch.isfinite(A0).all() and torch.isfinite(B0).all()
    ra = float(((A0.double() - wantA).abs().max() / (3e-6 * wantA.abs().max())).item())
    rb = float(((B0.double() - wantB).abs().max() / (3e-6 * wantB.abs().max())).item())
    _record("b.gram", tag, max(ra, rb))
    assert ra <= 1.0 and rb <= 1.0, (ra, rb)
    assert torch.equal(A0, A0.T)
    A2, B2 = _run_gram(ops, dx, da, dy, geom, bias, n)
    assert _same_bits(A0, A2) and _same_bits(B0, B2)
    ops._ws["gram"].fill_(0xFF)
    A3, B3 = _run_gram(ops, dx, da, dy, geom, bias, n)
    assert _same_bits(A0, A3) and _same_bits(B0, B3)
    if tag in ("finish-strided-3457", "E129", "rows-two-blocks-6-2"):
        # accumulate = 1 on top of a prior result: one fp32 addition per entry
        pa, pb = dev(torch.randn(n, n, generator=gen) * 100), dev(torch.randn(c2, n, generator=gen) * 100)
        A4, B4 = _run_gram(ops, dx, da, dy, geom, bias, n, prior=(pa, pb))
        assert _same_bits(A4, pa + A0) and _same_bits(B4, pb + B0)


# ------------------------------------------------------------------ c. effq_gram_accum_i8 / _unw
def _i8_scaled(ref, s, nw, bias, att):
    """What the finish kernel documents: A0 = 2 sc sum a k k^T, Au = sc sum k k^T with sc = (s | 1)(s | 1) per entry."""
    sv = torch.full((nw + int(bias),), s, dtype=torch.float64, device=ref["A"].device)
    if bias:
        sv[-1] = 1.0
    SC = sv[:, None] * sv[None, :]
    return 2.0 * SC * ref["A"], 2.0 * ref["B"] * sv[None, :], SC * ref["Au"], ref["Bu"] * sv[None, :]


def _check_i8(ops, tag, idx, y, att, cls, geom, k, s_, p, bias, alpha, La, cross_check=True):
    """gram_i8 on level ids `idx` [N, D, H, W, C1] uint8 against the fp64 (exact integer) reference."""
    nw = int(idx.shape[-1]) * int(np.prod(_t3(k)))
    ref = gram_reference(idx.float(), y, att, k, s_, p, bias, device=DEV)
    sa = float(np.float32(alpha)) / (La - 1)
    wantA, wantB, wantAu, wantBu = _i8_scaled(ref, sa, nw, bias, att)
    al = torch.tensor(alpha, dtype=torch.float32, device=DEV)
    didx, dy = dev(idx), dev(y)
    A0, B0, Au, Bu = ops.gram_i8(didx, cls, dy, geom, bias, al, La, unweighted=True)
    assert torch.equal(Au, wantAu), float((Au - wantAu).abs().max().item())          # the integer part is exact
    ra = float(((A0.double() - wantA).abs().max() / (2e-7 * wantA.abs().max())).item())    # fp32 output rounding only
    rb = float(((B0.double() - wantB).abs().max() / (2e-7 * wantB.abs().max())).item())
    ru = float(((Bu - wantBu).abs().max() / (2e-8 * wantBu.abs().max())).item())     # y rides in 32-bit fixed point
    _record("c.gram_i8", tag, max(ra, rb, ru))
    assert ra <= 1.0 and rb <= 1.0 and ru <= 1.0, (ra, rb, ru)
    assert torch.equal(A0, A0.T) and torch.equal(Au, Au.T)
    ops._ws["gram_i8"].fill_(0xFF)
    A2, B2, Au2, Bu2 = ops.gram_i8(didx, cls, dy, geom, bias, al, La, unweighted=True)
    assert _same_bits(A0, A2) and _same_bits(B0, B2) and _same_bits(Au, Au2) and _same_bits(Bu, Bu2)
    A3, B3 = ops.gram_i8(didx, cls, dy, geom, bias, al, La)                           # effq_gram_accum_i8 itself
    assert _same_bits(A0, A3) and _same_bits(B0, B3)
    if cross_check:
        xhat = (float(np.float32(alpha)) * idx.double() / (La - 1)).float()
        Af, Bf = ops.gram(dev(xhat), dev(att), dy, geom, bias)
        rf = max(float(((A0 - Af).abs().max() / (3e-6 * wantA.abs().max())).item()),
                 float(((B0 - Bf).abs().max() / (3e-6 * wantB.abs().max())).item()))
        _record("c.gram_i8 vs gram", tag, rf)
        assert rf <= 1.0, rf
    return A0, B0, wantA, wantB


@pytest.mark.parametrize("La,with_list", [(4, False), (16, True)], ids=["4levels-nolist", "16levels-list"])
def test_i8_gram_with_long_int32_partial_sums(ops, La, with_list):
    """A 32 -> 32, 3^3 layer at 2^20 voxels: 94 chunks of 128 voxels per split accumulate in int32 before each flush."""
    shape, c2, k = (4, 32, 64, 64, 64), 32, 3
    geom = _geom(shape, c2, k, 1, 1)
    assert ops.gram_i8_supported(geom, La)
    gen = torch.Generator().manual_seed(300 + La)
    idx = torch.randint(0, La, (shape[0], *shape[2:], shape[1]), generator=gen, dtype=torch.uint8)
    y = torch.randn(shape[0], *shape[2:], c2, generator=gen) * 3.7
    att, cls = None, (None, None, None, 1)
    if with_list:
        att = torch.tensor([1.0, 2.5, 17.25])[torch.randint(0, 3, (shape[0], *shape[2:]), generator=gen)]
        cls = ops.att_classes(dev(att))
        assert cls is not None and cls[3] == 3
    plan = ops.gram_i8_plan(geom, cls[3], 0 if cls[0] is None else cls[0].numel())
    assert plan["cps"] >= 64 and plan["nsplit"] >= 64 and plan["NB"] == 8 and plan["NBX"] == 7, plan
    assert plan["cps"] * 128 * (La - 1) ** 2 < 2 ** 31
    _check_i8(ops, f"2^20 voxels La={La} {plan}", idx, y, att, cls, geom, k, 1, 1, True, 0.7312, La)


def test_i8_gram_at_the_largest_level_id(ops):
    """16 -> 16, 1^3 at 128 levels and 2^21 voxels with EVERY id at 127: each int32 partial sum of a split reaches
    cps * 128 * 127^2, the largest value the planned chunk count allows."""
    shape, c2, La = (1, 16, 128, 128, 128), 16, 128
    geom = _geom(shape, c2, 1, 1, 0)
    plan = ops.gram_i8_plan(geom)
    assert plan["npairs"] == 1 and plan["cps"] >= 4 and plan["nsplit"] > 1000, plan
    gen = torch.Generator().manual_seed(77)
    idx = torch.full((1, 128, 128, 128, 16), 127, dtype=torch.uint8)
    y = torch.randn(1, 128, 128, 128, c2, generator=gen)
    _check_i8(ops, f"ids 127 {plan}", idx, y, None, (None, None, None, 1), geom, 1, 1, 0, False, 1.27, La)


def _pad128(v):
    pad = (-v.numel()) % 128
    return torch.cat([v, torch.full((pad,), -1, dtype=torch.int32)])


def test_i8_gram_class_structure_on_a_multi_block_system(ops):
    """16 classes on the 8 macro blocks of a 32 -> 32, 3^3 system: a class of 5 voxels, classes of exactly 128 and 256
    voxels, three weights present in the first volume only (sharded accumulation then sees other class tables per call),
    and a hand-made list whose middle class is empty."""
    shape, c2, k, La = (2, 32, 8, 9, 10), 32, 3, 4
    geom = _geom(shape, c2, k, 1, 1)
    per = 8 * 9 * 10
    gen = torch.Generator().manual_seed(55)
    others = torch.tensor([1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0])
    rest0 = others[torch.cat([torch.arange(13), torch.randint(0, 13, (per - 5 - 128 - 256 - 13,), generator=gen)])]
    v0 = torch.cat([torch.full((5,), 0.25), torch.full((128,), 12.0), torch.full((256,), 0.5), rest0])
    v0 = v0[torch.randperm(per, generator=gen)]
    v1 = others[torch.cat([torch.arange(13), torch.randint(0, 13, (per - 13,), generator=gen)])]
    att = torch.stack([v0, v1[torch.randperm(per, generator=gen)]]).reshape(2, 8, 9, 10)
    idx = torch.randint(0, La, (2, 8, 9, 10, 32), generator=gen, dtype=torch.uint8)
    y = torch.randn(2, 8, 9, 10, c2, generator=gen) * 3.7
    cls = ops.att_classes(dev(att))
    assert cls is not None and cls[3] == 16
    sizes = torch.bincount(cls[1].cpu()).tolist()
    assert sizes[0] == 1 and sizes[1] == 2 and sizes[-1] == 1, sizes          # 0.25: 5 voxels, 0.5: 256, 12.0: 128
    plan = ops.gram_i8_plan(geom, 16, cls[0].numel())
    assert plan["NB"] == 8 and plan["nchunks"] == cls[0].numel() // 128, plan
    A0, B0, wantA, wantB = _check_i8(ops, "16 classes", idx, y, att, cls, geom, k, 1, 1, True, 0.7312, La)
    # sharded over the volumes: 16 classes in the first call, 13 in the second
    al = torch.tensor(0.7312, dtype=torch.float32, device=DEV)
    g1 = _geom((1,) + shape[1:], c2, k, 1, 1)
    c0, c1 = ops.att_classes(dev(att[:1].contiguous())), ops.att_classes(dev(att[1:].contiguous()))
    assert c0[3] == 16 and c1[3] == 13
    A1, B1 = ops.gram_i8(dev(idx[:1]), c0, dev(y[:1]), g1, True, al, La)
    A1, B1 = ops.gram_i8(dev(idx[1:]), c1, dev(y[1:]), g1, True, al, La, A1, B1)
    assert (A1 - A0).abs().max() <= 3e-7 * wantA.abs().max() and (B1 - B0).abs().max() <= 3e-7 * wantB.abs().max()
    # an empty class between two used ones (the list format allows it: chunk_cls names classes 0 and 2 only)
    flat = att.reshape(-1)
    lo = torch.nonzero(flat < 3.0).reshape(-1).to(torch.int32)
    hi = torch.nonzero(flat >= 3.0).reshape(-1).to(torch.int32)
    lst = torch.cat([_pad128(lo), _pad128(hi)])
    chunk_cls = torch.cat([torch.zeros(_pad128(lo).numel() // 128, dtype=torch.int32),
                           torch.full((_pad128(hi).numel() // 128,), 2, dtype=torch.int32)])
    att3 = torch.where(flat < 3.0, torch.tensor(1.75), torch.tensor(0.375)).reshape(att.shape)
    cls3 = (dev(lst), dev(chunk_cls), dev(torch.tensor([1.75, 99.0, 0.375])), 3)
    _check_i8(ops, "empty middle class", idx, y, att3, cls3, geom, k, 1, 1, True, 0.7312, La, cross_check=False)


# ------------------------------------------------------------------ d. effq_gram_loss, effq_gram_loss_i8
@pytest.mark.parametrize("n,c2,bias", [(3457, 128, True), (6913, 256, True), (3457, 100, True), (1728, 45, False)],
                         ids=["n3457-c128", "n6913-c256", "n3457-c100", "n1728-c45-nobias"])
def test_fp64_loss_on_the_wide_systems(ops, n, c2, bias):
    """effq_gram_loss on a synthetic SPD Au and a random Bu against the same quadratic form by fp64 matrix products:
    |got - want| <= max(1e-10 want, n^2 2^-53 (sum_c |g|^T |Au| |g| + 2 sum |g . Bu| terms + syy))."""
    gen = torch.Generator().manual_seed(n + c2)
    M = dev(torch.randn(n, 48, generator=gen)).double()
    Au = M @ M.T + torch.eye(n, dtype=torch.float64, device=DEV)
    Bu = dev(torch.randn(c2, n, generator=gen)).double() * 3
    nw = n - int(bias)
    G = dev(torch.randn(c2, nw, generator=gen) * 0.05)
    b = dev(torch.randn(c2, generator=gen) * 0.1) if bias else None
    syy = torch.tensor([float(c2 * n) * 7.5], dtype=torch.float64, device=DEV)
    g = torch.cat([G.double(), b.double()[:, None]], 1) if bias else G.double()
    want = float((((g @ Au) * g).sum() - 2 * (g * Bu).sum() + syy[0]).item())
    mag = float((((g.abs() @ Au.abs()) * g.abs()).sum() + 2 * (g * Bu).abs().sum() + syy[0]).item())
    bound = max(1e-10 * abs(want), n * n * U53 * mag)
    got = ops.gram_loss(Au, Bu, syy, G, b).cpu().tolist()
    assert got[0] == got[1]
    _record("d.gram_loss", f"n={n} c2={c2}", abs(got[0] - want) / bound)
    print(f"   (1e-10 want = {1e-10 * abs(want):.3g}, derived bound = {n * n * U53 * mag:.3g}, error = {abs(got[0] - want):.3g})")
    assert abs(got[0] - want) <= bound, (got, want, bound)
    assert ops.gram_loss(Au, Bu, syy, G, b).cpu().tolist() == got


def _flag(planes):
    torch.cuda.synchronize()
    return int(planes._effq_err.item())


def plane_capacity(P):
    """Largest non-negative integer P balanced base-256 digits (-128 .. 127) hold."""
    return 127 * ((256 ** P - 1) // 255)


def _synthetic_k(nw, kmax, gen):
    """A symmetric integer matrix of small entries with `kmax` on the diagonal, inside the first diagonal tile (another
    64-column chunk where there is one) and, mirrored, in the farthest off-diagonal corner; the big entries as a dict."""
    Ks = torch.randint(-100, 101, (nw, nw), generator=gen, dtype=torch.int16)
    Ks = dev(Ks).to(torch.int64)
    Ks = torch.triu(Ks) + torch.triu(Ks, 1).T
    big = {(3, 3): kmax, (nw - 2, nw - 2): kmax - 1, (10, nw - 3): kmax, (5, min(nw - 1, 70)): -(kmax // 2)}
    K = Ks.clone()
    for (i, j), v in big.items():
        Ks[i, j] = Ks[j, i] = 0
        K[i, j] = K[j, i] = v
    return K, Ks, big


def _exact_q(Ks, big, Jq):
    """<K, J^T J> as a Python int: the small part of K in fp64 (every partial sum is an integer below 2^53: 100 * 9 c2 nw^2),
    the few large entries in Python integers."""
    J = Jq.double()
    Mm = J.T @ J
    q = int((Ks.double() * Mm).sum().item())
    for (i, j), v in big.items():
        q += (1 if i == j else 2) * v * int(Mm[i, j].item())
    return q


def _levels_to_j(lv, Lw):
    return (2 * lv - (Lw - 1)).to(torch.int8)


# nw, c2, count, planes: (count * c2 = 32: one partial column tile; 288: one above a multiple of 256)
GL8_CASES = [(64, 32, 1, 1), (64, 32, 16, 4), (320, 32, 9, 5), (1728, 64, 5, 6), (6912, 32, 9, 4), (6912, 128, 2, 5)]


@pytest.mark.parametrize("nw,c2,count,P", GL8_CASES, ids=[f"nw{c[0]}-c{c[1]}-x{c[2]}-P{c[3]}" for c in GL8_CASES])
@pytest.mark.parametrize("edge", ["at-capacity", "above-capacity"])
def test_i8_loss_digit_planes_and_group_shapes(ops, nw, c2, count, P, edge):
    """effq_gram_loss_i8 on Au = s^2 K for a synthetic symmetric integer K whose largest entry is the capacity of P digit
    planes (127 (256^P - 1) / 255) or one above it (P + 1 planes; none at P = 6).  The planes reproduce K, the quadratic
    form <K, J^T J> equals the exact integer (no cross terms: s_w = 1, s_a = 1/4 make the fp64 scaling exact), and with a
    bias row, Bu and syy the loss meets the 2e-8 of the existing test."""
    Lw, La, alpha = 4, 2, 0.25
    kmax = plane_capacity(P) + (1 if edge == "above-capacity" else 0)
    want_P = P if edge == "at-capacity" else P + 1
    assert ops.lib.effq_gram_loss_i8_num_planes(kmax) == (want_P if want_P <= 6 else -1)
    assert ops.lib.effq_gram_loss_i8_num_planes((1 << (8 * P - 1)) - 1) == (P if P == 1 else (P + 1 if P < 6 else -1))
    assert ops.gram_loss_i8_supported(c2, nw, False, Lw) and ops.gram_loss_i8_supported(c2, nw + 1, True, Lw)
    mt, nt = -(-nw // 256), -(-(count * c2) // 256)
    gen = torch.Generator().manual_seed(nw + c2 + count + P)
    al = torch.tensor(alpha, dtype=torch.float32, device=DEV)
    K, Ks, big = _synthetic_k(nw, kmax, gen)
    s2 = alpha * alpha                                          # 1/16: Au is exact
    Au = K.double() * s2
    planes = ops.gram_loss_i8_planes(Au, False, al, La, kmax)
    if want_P > 6:
        assert planes is None
        # too few planes for the entries: the flag says so (the digits are cut, nothing else happens)
        planes = ops.gram_loss_i8_planes(Au, False, al, La, plane_capacity(6))
        torch.cuda.synchronize()
        assert planes.shape[0] == 6 and _flag(planes) == 2
        return
    torch.cuda.synchronize()
    assert planes.shape[0] == want_P and _flag(planes) == 0
    assert planes.shape[1] == mt * 256 and mt * want_P * nt >= 1
    Kp = sum((256 ** q) * planes[q, :nw].to(torch.int64) for q in range(want_P))
    assert torch.equal(Kp, K) and not bool(planes[:, nw:].any().item())
    # iterates: random level ids of 4 weight levels, weight scale 3 -> s_w = 1
    Jq = _levels_to_j(torch.randint(0, Lw, (count, c2, nw), generator=gen), Lw)
    dJ = dev(Jq)
    states = torch.zeros(count, 5, dtype=torch.float64, device=DEV)
    states[:, 0] = 3.0
    zero_B = torch.zeros(c2, nw, dtype=torch.float64, device=DEV)
    zero = torch.zeros(1, dtype=torch.float64, device=DEV)
    hist = ops.gram_loss_i8(planes, Au, zero_B, zero, dJ, None, states, al, La, Lw).cpu().numpy()
    exact = [_exact_q(Ks, big, dJ[j]) for j in range(count)]
    assert all(abs(q) < 2 ** 62 for q in exact)
    assert [float(h) for h in hist[:, 0]] == [float(q) * s2 for q in exact], (hist[:, 0], exact)
    assert np.array_equal(hist[:, 0], hist[:, 1])
    # with the bias row, Bu and syy: n = nw + 1
    n = nw + 1
    Ab = torch.zeros(n, n, dtype=torch.float64, device=DEV)
    Ab[:nw, :nw] = Au
    col = dev(torch.randint(0, 1000, (nw,), generator=gen)).double() * alpha
    Ab[:nw, nw] = col
    Ab[nw, :nw] = col
    Ab[nw, nw] = 4000.0
    Bu = dev(torch.randn(c2, n, generator=gen)).double() * 50
    syy = torch.tensor([float(kmax) * 10.0 + 1e6], dtype=torch.float64, device=DEV)
    b = dev(torch.randn(count, c2, generator=gen) * 0.1)
    pl_b = ops.gram_loss_i8_planes(Ab, True, al, La, kmax)
    torch.cuda.synchronize()
    assert _flag(pl_b) == 0 and torch.equal(pl_b, planes)
    got = ops.gram_loss_i8(pl_b, Ab, Bu, syy, dJ, b, states, al, La, Lw).cpu().numpy()
    worst = 0.0
    for j in range(count):
        g = torch.cat([dJ[j].double(), b[j].double()[:, None]], 1)
        lin = float(((2 * g[:, :nw] * g[:, nw:] * col[None, :]).sum() + (g[:, nw] ** 2).sum() * 4000.0
                     - 2 * (g * Bu).sum() + syy[0]).item())
        want = float(exact[j]) * s2 + lin
        mag = abs(float(exact[j]) * s2) + abs(lin)
        worst = max(worst, abs(got[j, 0] - want) / (2e-8 * mag))
        assert abs(got[j, 0] - want) <= 2e-8 * mag, (j, got[j, 0], want)
    _record("d.gram_loss_i8", f"nw={nw} c2={c2} x{count} P={want_P}", worst)


def test_i8_loss_prepare_flags_what_is_not_an_integer_system(ops):
    """effq_gram_loss_i8_prepare raises its flag for an entry that is no integer multiple of s^2 (1) and for entries beyond
    the planes it was given (2), and leaves it clear otherwise."""
    al = torch.tensor(0.25, dtype=torch.float32, device=DEV)
    gen = torch.Generator().manual_seed(5)
    K, _, _ = _synthetic_k(64, plane_capacity(2), gen)
    Au = K.double() / 16
    assert _flag(ops.gram_loss_i8_planes(Au, False, al, 2, plane_capacity(2))) == 0
    assert _flag(ops.gram_loss_i8_planes(Au, False, al, 2, plane_capacity(1))) == 2
    # 2^15 - 1 does NOT fit two balanced digits (32639 is the most): the planner must not promise it does
    K[7, 9] = K[9, 7] = 32767
    pl = ops.gram_loss_i8_planes(K.double() / 16, False, al, 2, 32767)
    assert pl.shape[0] == 3 and _flag(pl) == 0
    # ... and the kernel agrees: told to use two planes, it carries out of the top digit at 32640 and not at 32639
    from efficientq_amd.hip_ops import _ptr
    from efficientq_amd._lib import check
    for top, flag in ((32639, 0), (32640, 2), (32767, 2)):
        K[7, 9] = K[9, 7] = top
        two = torch.empty(2, 256, 64, dtype=torch.int8, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        check(ops.lib.effq_gram_loss_i8_prepare(_ptr(K.double() / 16), 64, 0, _ptr(al), 2, 2, _ptr(two), _ptr(err),
                                                ops.stream), "effq_gram_loss_i8_prepare")
        torch.cuda.synchronize()
        assert int(err.item()) == flag, (top, int(err.item()))
        if flag == 0:
            assert torch.equal(two[0, :64].to(torch.int64) + 256 * two[1, :64].to(torch.int64), K)
    bad = Au.clone()
    bad[20, 21] += 0.4 / 16
    assert _flag(ops.gram_loss_i8_planes(bad, False, al, 2, plane_capacity(2))) == 1


def test_i8_loss_three_groups_on_one_workspace(ops):
    """Three groups of different sizes in a row on the library's workspace, never zeroed in between: the kernels leave the
    tile ticket, the per-iterate tickets and Qacc at zero."""
    nw, c2, Lw, La, alpha = 320, 64, 4, 2, 0.25
    gen = torch.Generator().manual_seed(9)
    al = torch.tensor(alpha, dtype=torch.float32, device=DEV)
    K, Ks, big = _synthetic_k(nw, plane_capacity(3), gen)
    Au = K.double() / 16
    planes = ops.gram_loss_i8_planes(Au, False, al, La, plane_capacity(3))
    zero_B = torch.zeros(c2, nw, dtype=torch.float64, device=DEV)
    zero = torch.zeros(1, dtype=torch.float64, device=DEV)
    for count in (16, 1, 5):
        dJ = dev(_levels_to_j(torch.randint(0, Lw, (count, c2, nw), generator=gen), Lw))
        states = torch.zeros(count, 5, dtype=torch.float64, device=DEV)
        states[:, 0] = 3.0
        hist = ops.gram_loss_i8(planes, Au, zero_B, zero, dJ, None, states, al, La, Lw).cpu().numpy()
        assert [float(h) for h in hist[:, 0]] == [float(_exact_q(Ks, big, dJ[j])) / 16 for j in range(count)], count
    ws = ops._ws["gram_loss_i8"]
    torch.cuda.synchronize()
    assert not bool(ws[:128 + 64 + 4].any().item())           # Qacc [16], tickets [16], the tile ticket
