"""The persistent conv kernels where every workgroup walks several output tiles, against fp64.

Every conv kernel walks the tiles [b * per, min((b + 1) * per, ntiles)) with per = ceil(ntiles / grid.x), prefetching the
next tile's halo and targets while it computes the current one.  The planners clamp grid.x to ntiles, so at the sizes of
test_hip_kernels.py every workgroup computes exactly one tile.  The cases here have more output tiles than the largest
grid.x the planner can give the kernel they select (per >= 2), so they reach the cross-tile prefetch, the clipped last run
and, where noted, workgroups with no tile at all that must still post a zero partial sum.

Runs on a real MI355X only (-m gpu)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_ops(DEV)


def _cdiv(a, b):
    return -(-a // b)


def _triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(v)


def _out_dims(sp, k, s, p):
    return tuple((d + 2 * pp - kk) // ss + 1 for d, kk, ss, pp in zip(sp, _triple(k), _triple(s), _triple(p)))


def _ntiles(n, out, tile):
    return n * _cdiv(out[0], tile[0]) * _cdiv(out[1], tile[1]) * _cdiv(out[2], tile[2])


def _ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def _poison(shape):
    """NaN-fill a block of the output's size and free it: the caching allocator hands that block to the next allocation of
    the same size on this stream, so an output voxel that no workgroup writes stays NaN.  Returns the block's address."""
    t = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    ptr = t.data_ptr()
    del t
    return ptr


def _check_poisoned(out, ptr):
    assert out.data_ptr() == ptr, "the output did not land in the NaN-filled block"
    assert bool(torch.isfinite(out).all()), f"{int((~torch.isfinite(out)).sum())} output values never written"


def _close(got, want, rel):
    return abs(got - want) <= rel * abs(want)


# ------------------------------------------------------------------ f32 path: conv3d_quant_calib_step
# Tiled kernels (conv3d.hip make_plan): 4 x 4 x 8-voxel output tiles; nsub = C2 / 32 output blocks, NT = 2 of them per wave
# when nsub is even and ntiles * nsub / 2 >= 1024 (else NT = 1); ny = nsub / NT; grid.x = min(ntiles, max(64, ceil(512 / ny))).
# So per >= 2 once ntiles > max(64, ceil(512 / ny)): 512 for ny = 1, 256 for ny = 2, 128 for ny = 4.
# 3^3 / stride 1 / C1, C2 multiples of 32 take k_conv3d_k3<NT, *>, every other shape k_conv3d<NT, C1 % 4 == 0, *>.
# Loss-only calls without mask or fused quantiser of the first convs go to the direct-gather kernels (conv3d_direct.hip
# conv_direct_launch): same 4 x 4 x 8 tiles, grid.x = min(ntiles, 512); 4 -> 32 -> k_conv3d_c4h<S>, 1 -> 32 -> k_conv3d_c1h<S>.
F32_CASES = {
    # id: (c1, c2, k, stride, pad, N, input spatial)
    # 605 tiles, ny = 1, grid 512: per 2, the last run clipped to one tile, 209 idle workgroups
    "k3_32to32": (32, 32, 3, 1, 1, 1, (43, 42, 37)),
    # 315 tiles < 1024 so NT = 1, ny = 2, grid 256: per 2, 158 busy (last run clipped), 98 idle
    "k3_64to64": (64, 64, 3, 1, 1, 1, (20, 36, 56)),
    # 1430 tiles >= 1024 so NT = 2, ny = 1, grid 512: per 3, 477 busy (last run 2 tiles), 35 idle
    "k3_64to64_nt2": (64, 64, 3, 1, 1, 1, (44, 40, 104)),
    # 150 tiles < 512 so NT = 1, ny = 4, grid 128: per 2, 75 busy, 53 idle
    "k3_128to128": (128, 128, 3, 1, 1, 1, (20, 24, 40)),
    # the same grid, 8 channel slabs per tile: the next tile's slab 0 is prefetched behind slab 7
    "k3_256to128": (256, 128, 3, 1, 1, 1, (20, 24, 40)),
    # 260 tiles >= 256 so NT = 2, ny = 4, grid 128: per 3, 87 busy (last run 2 tiles), 41 idle
    "k3_128to256_nt2": (128, 256, 3, 1, 1, 1, (20, 52, 32)),
    # first conv, stride 2: 44 x 44 x 40 out, 605 tiles, grid 512 (k_conv3d<1, vec> and k_conv3d_c4h<2>): per 2, 209 idle
    "first_4to32_s2": (4, 32, 3, 2, 1, 1, (88, 88, 80)),
    # the same at stride 1 (k_conv3d<1, vec> and k_conv3d_c4h<1>)
    "first_4to32_s1": (4, 32, 3, 1, 1, 1, (44, 44, 40)),
    # single-modality first conv, the LiTS stride (k_conv3d<1, novec> and k_conv3d_c1h<2, 2, 1>): 605 tiles, grid 512
    "first_1to32_s221": (1, 32, 3, (2, 2, 1), 1, 1, (88, 88, 40)),
    # stride 2 and stride 1 (k_conv3d_c1h<2, 2, 2>, k_conv3d_c1h<1, 1, 1>)
    "first_1to32_s2": (1, 32, 3, 2, 1, 1, (88, 88, 80)),
    "first_1to32_s1": (1, 32, 3, 1, 1, 1, (44, 44, 40)),
    # generic NT = 2, vec: 1x1x1, 605 tiles >= 512 so NT = 2, ny = 2, grid 256: per 3, 202 busy (last run 2 tiles), 54 idle
    "k1_64to128_nt2": (64, 128, 1, 1, 0, 1, (43, 42, 37)),
    # generic NT = 2, C1 % 4 != 0: 1430 tiles >= 1024 so NT = 2, ny = 1, grid 512: per 3, 477 busy, 35 idle
    "k3_2to64_nt2": (2, 64, 3, 1, 1, 1, (44, 40, 104)),
}


def _f32_grid_bound(c2, ntiles):
    """Largest grid.x make_plan can give a tiled kernel of this output width (see the comment above F32_CASES)."""
    nsub = _cdiv(c2, 32)
    nt = 2 if nsub % 2 == 0 and ntiles * (nsub // 2) >= 1024 else 1
    return max(64, _cdiv(512, nsub // nt))


def _direct_kind(c1, c2, k):
    return c2 == 32 and k == 3 and c1 in (1, 4)


def _f32_problem(case, seed):
    c1, c2, k, s, p, n, sp = F32_CASES[case]
    out = _out_dims(sp, k, s, p)
    nt = _ntiles(n, out, (4, 4, 8))
    assert nt > _f32_grid_bound(c2, nt), "the case must give every workgroup more than one tile"
    if _direct_kind(c1, c2, k):
        assert nt > 512
    gen = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(n, c1, *sp, generator=gen))
    w = torch.randn(c2, c1, k, k, k, generator=gen) * (1.0 / (c1 * k ** 3) ** 0.5)
    b = torch.randn(c2, generator=gen) * 0.1
    att = torch.tensor([0.25, 1.0, 3.5])[torch.randint(0, 3, (n, *out), generator=gen)]
    noise = torch.randn(n, c2, *out, generator=gen)
    return (c1, c2, k, s, p), x, w, b, att, noise


def _sums_vs_fp64(sq, ref, y, att, rel=1e-5):
    d2 = (ref - y.double()) ** 2
    s0 = d2.sum().item()
    s1 = (att.double().unsqueeze(1) * d2).sum().item() if att is not None else s0
    got = sq.cpu().tolist()
    assert _close(got[0], s0, rel) and _close(got[1], s1, rel), (got, s0, s1)
    return got


@pytest.mark.parametrize("case", list(F32_CASES))
def test_conv_step_walks_several_tiles_per_workgroup(ops, case):
    """Output only, loss only (with and without the mask) and both, with and without bias, against F.conv3d in fp64."""
    from efficientq_amd.hip_ops import make_geom
    (c1, c2, k, s, p), x, w, b, att, noise = _f32_problem(case, seed=sum(map(ord, case)))
    ref = F.conv3d(x.double(), w.double(), b.double(), s, p)
    y = (ref + 0.1 * noise.double()).float()
    geom = make_geom(x.shape, c2, k, s, p)
    xs, ws, bs, ys, atts = (t.to(DEV) for t in (_ndhwc(x), w, b, _ndhwc(y), att))
    oshape = (ref.shape[0], *ref.shape[2:], c2)
    scale = ref.abs().max().item()

    # output only (k_conv3d*<..., noY>), with and without bias
    ptr = _poison(oshape)
    out, sq = ops.conv_step(xs, ws, bs, geom, want_out=True)
    assert sq is None
    _check_poisoned(out, ptr)
    assert (_ncdhw(out).cpu().double() - ref).abs().max().item() <= 1e-5 * scale
    ptr = _poison(oshape)
    out, _ = ops.conv_step(xs, ws, None, geom, want_out=True)
    _check_poisoned(out, ptr)
    ref_nb = ref - b.double().view(1, -1, 1, 1, 1)
    assert (_ncdhw(out).cpu().double() - ref_nb).abs().max().item() <= 1e-5 * ref_nb.abs().max().item()

    # loss only with the mask (tiled kernel), twice: bit-identical
    _, sq_a = ops.conv_step(xs, ws, bs, geom, ys, atts)
    la = _sums_vs_fp64(sq_a, ref, y, att)
    _, sq_a2 = ops.conv_step(xs, ws, bs, geom, ys, atts)
    assert sq_a2.cpu().tolist() == la

    # loss only without the mask (the direct-gather kernels for the first convs), twice: bit-identical
    _, sq_n = ops.conv_step(xs, ws, bs, geom, ys, None)
    ln = _sums_vs_fp64(sq_n, ref, y, None)
    assert ln[1] == ln[0]
    _, sq_n2 = ops.conv_step(xs, ws, bs, geom, ys, None)
    assert sq_n2.cpu().tolist() == ln
    if not _direct_kind(c1, c2, k):
        assert ln[0] == la[0]             # same tiled kernel, same summation order

    # bias-free loss only
    _, sq_nb = ops.conv_step(xs, ws, None, geom, ys, atts)
    _sums_vs_fp64(sq_nb, ref_nb, y, att)

    # output and loss in one call: the output-only values and the loss-only sums
    ptr = _poison(oshape)
    out, sq_b = ops.conv_step(xs, ws, bs, geom, ys, atts, want_out=True)
    _check_poisoned(out, ptr)
    assert (_ncdhw(out).cpu().double() - ref).abs().max().item() <= 1e-5 * scale
    assert sq_b.cpu().tolist() == la


@pytest.mark.parametrize("case,levels,with_att,with_bias", [
    ("k3_32to32", 4, True, True), ("k3_64to64_nt2", 16, False, False), ("k3_128to256_nt2", 4, True, False),
    ("first_4to32_s2", 4, False, True), ("first_1to32_s221", 16, True, True), ("k3_2to64_nt2", 4, True, False)])
def test_conv_step_fused_act_quant_walks_several_tiles(ops, case, levels, with_att, with_bias):
    """The activation quantiser fused into the halo staging equals the unfused call on quant_dequant_f32(x) bit for bit
    (output and sums), and both match fp64 on the quantised input."""
    from efficientq_amd.hip_ops import make_geom
    (c1, c2, k, s, p), x, w, b, att, noise = _f32_problem(case, seed=3 + sum(map(ord, case)))
    alpha = torch.tensor(0.8123)
    geom = make_geom(x.shape, c2, k, s, p)
    xs = _ndhwc(x).to(DEV)
    xq = ops.quant_dequant_f32(xs, alpha.to(DEV), levels, 0.0, 1.0)
    bb = b if with_bias else None
    ref = F.conv3d(_ncdhw(xq).cpu().double(), w.double(), None if bb is None else bb.double(), s, p)
    y = (ref + 0.1 * noise.double()).float()
    a = att if with_att else None
    ws, bs, ys = w.to(DEV), None if bb is None else bb.to(DEV), _ndhwc(y).to(DEV)
    atts = None if a is None else a.to(DEV)
    oshape = (ref.shape[0], *ref.shape[2:], c2)
    out_u, sq_u = ops.conv_step(xq, ws, bs, geom, ys, atts, want_out=True)
    ptr = _poison(oshape)
    out_f, sq_f = ops.conv_step(xs, ws, bs, geom, ys, atts, act_alpha=alpha.to(DEV), act_levels=levels, want_out=True)
    _check_poisoned(out_f, ptr)
    assert torch.equal(out_f, out_u)
    lf = sq_f.cpu().tolist()
    assert lf == sq_u.cpu().tolist()
    assert (_ncdhw(out_f).cpu().double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    _sums_vs_fp64(sq_f, ref, y, a)
    # loss only, fused: the same sums again
    _, sq_l = ops.conv_step(xs, ws, bs, geom, ys, atts, act_alpha=alpha.to(DEV), act_levels=levels)
    assert sq_l.cpu().tolist() == lf


# ------------------------------------------------------------------ exact-integer paths: conv3d_calib_step_i8 / _forward_i8
# i8_plan (conv3d_i8.hip): output tiles of 8 x 4 x 8 voxels for C1 = 32, 2 x 4 x 8 for C1 = 512, 4 x 4 x 8 otherwise;
# ny = C2 / 32 (C2 / 64 for C1 = 512), wg = 2 workgroups per CU for C1 in {32, 128}, else 1; gx = max(32, ceil(256 wg / ny));
# when gx * ny > 30 the grid keeps 15 slots free: g0 = gx - ceil(15 / ny), per = ceil(ntiles / g0), grid.x = ceil(ntiles / per)
# (equal runs, no idle workgroup, the last run clipped).  So per >= 2 once ntiles > g0, per >= 3 once ntiles > 2 g0.
# k_conv3d_i8w (64 -> 64, tile-divisible output) ignores that grid: grid.x = min(ntiles, 256), so per >= 2 above 256 tiles
# and idle workgroups whenever 256 does not divide into runs of per tiles.
I8_CASES = {
    # id: (c1, c2, N, spatial (3^3, pad 1: output = input), act levels, weight levels, bias)
    # k_conv3d_i8l2e: 1210 tiles > 2 * 497: per 3, grid 404, the last run one tile (A/B register sets reused)
    "l2e_32to32": (32, 32, 2, (40, 44, 88), 4, 4, True),
    # k_conv3d_i8l2 (32 -> 64, ragged H): 605 tiles, g0 = 248: per 3, grid 202, the last run two tiles
    "l2_32to64": (32, 64, 1, (40, 42, 84), 16, 16, False),
    # k_conv3d_i8<2> (64 -> 64, ragged): 256 tiles, g0 = 120: per 3, grid 86, the last run one tile
    "i8_64to64_ragged": (64, 64, 1, (30, 30, 30), 4, 4, True),
    # k_conv3d_i8w (64 -> 64, even): 660 tiles, grid 256: per 3, 220 busy, 36 idle
    "i8w_64to64": (64, 64, 1, (24, 40, 88), 4, 4, True),
    # k_conv3d_i8g<4> (128 -> 128): 175 tiles, g0 = 124: per 2, grid 88, the last run one tile
    "i8g4_128to128": (128, 128, 1, (20, 20, 56), 4, 4, True),
    # k_conv3d_i8g<8> (256 -> 128): 75 tiles, g0 = 60: per 2, grid 38, the last run one tile
    "i8g8_256to128": (256, 128, 1, (12, 20, 40), 16, 4, False),
    # k_conv3d_i8g2<16> (512 -> 256): 2 x 4 x 8 tiles, 75 of them, g0 = 60: per 2, grid 38, the last run one tile
    "i8g2_512to256": (512, 256, 1, (6, 20, 40), 4, 4, True),
}


def _i8_tile(c1):
    return (8, 4, 8) if c1 == 32 else (2, 4, 8) if c1 == 512 else (4, 4, 8)


def _i8_w64(c1, c2, sp):
    return c1 == 64 and c2 == 64 and sp[0] % 4 == 0 and sp[1] % 4 == 0 and sp[2] % 8 == 0


def _i8_grid_bound(c1, c2, sp):
    """Largest grid.x i8_plan / the k_conv3d_i8w launch can give (see the comment above I8_CASES)."""
    if _i8_w64(c1, c2, sp):
        return 256
    ny = c2 // 64 if c1 == 512 else c2 // 32
    wg = 2 if c1 in (32, 128) else 1
    gx = max(32, _cdiv(256 * wg, ny))
    return gx - _cdiv(15, ny) if gx * ny > 30 else gx


def _i8_problem(ops, case, seed):
    c1, c2, n, sp, la, lw, with_bias = I8_CASES[case]
    nt = _ntiles(n, sp, _i8_tile(c1))
    assert nt > _i8_grid_bound(c1, c2, sp), "the case must give every workgroup more than one tile"
    gen = torch.Generator().manual_seed(seed)
    xidx = torch.randint(0, la, (n, *sp, c1), generator=gen, dtype=torch.uint8)
    gq = (2 * torch.randint(0, lw, (c2, c1, 3, 3, 3), generator=gen) - (lw - 1)).to(torch.int8)
    a_act = np.float32(0.8123)
    a_w = np.float32(3.0 / (27 * c1) ** 0.5)            # outputs of order one
    b = torch.randn(c2, generator=gen) * 0.1 if with_bias else None
    y = torch.randn(n, *sp, c2, generator=gen)
    att = torch.tensor([0.25, 1.0, 3.5])[torch.randint(0, 3, (n, *sp), generator=gen)]
    # the integer model in fp64 (exact for these sums): conv(level ids, numerators) * f32(a_a) f32(a_w) / ((La-1)(Lw-1)) + b
    ref = F.conv3d(xidx.permute(0, 4, 1, 2, 3).double(), gq.double(), None, 1, 1)
    ref = ref * (float(a_act) * float(a_w) / ((la - 1) * (lw - 1)))
    if b is not None:
        ref = ref + b.double().view(1, -1, 1, 1, 1)
    st = ops.new_fp_state()
    st[0] = float(a_w)
    dev = dict(xidx=xidx.to(DEV), gq=gq.to(DEV), b=None if b is None else b.to(DEV), y=y.to(DEV),
               alpha=torch.tensor(a_act, device=DEV), st=st)
    return (c1, c2, n, sp, la, lw), gq, a_w, y, att, ref, dev


def _i8_sums_vs_fp64(sq, ref, y, att):
    return _sums_vs_fp64(sq, ref, _ncdhw(y), att, rel=1e-6)


@pytest.mark.parametrize("case", list(I8_CASES))
def test_exact_int_conv_step_walks_several_tiles_per_workgroup(ops, case):
    """conv3d_calib_step_i8 on each kernel of the exact-integer loss: both sums against the fp64 integer model, a
    repeated call bit-identical."""
    from efficientq_amd.hip_ops import make_geom
    (c1, c2, n, sp, la, lw), _, _, y, _, ref, d = _i8_problem(ops, case, seed=5 + sum(map(ord, case)))
    geom = make_geom((n, c1, *sp), c2, 3, 1, 1)
    assert ops.conv_i8_supported(geom, la, lw)
    sq = torch.zeros(2, dtype=torch.float64, device=DEV)
    ops.conv_step_i8(d["xidx"], d["gq"], d["b"], geom, d["y"], d["alpha"], la, d["st"], lw, sq)
    got = _i8_sums_vs_fp64(sq, ref, y, None)
    assert got[1] == got[0]
    sq2 = torch.zeros(2, dtype=torch.float64, device=DEV)
    ops.conv_step_i8(d["xidx"], d["gq"], d["b"], geom, d["y"], d["alpha"], la, d["st"], lw, sq2)
    assert sq2.cpu().tolist() == got


@pytest.mark.parametrize("case,with_att", [("l2e_32to32", True), ("l2e_32to32", False),
                                           ("i8w_64to64", True), ("i8w_64to64", False)])
def test_quantised_forward_walks_several_tiles_per_workgroup(ops, case, with_att):
    """conv3d_quant_forward_i8 (k_conv3d_i8l2e<true>, k_conv3d_i8w<true>): every output voxel written, output and sums
    against the fp64 integer model, a repeated call bit-identical."""
    from efficientq_amd.hip_ops import make_geom
    (c1, c2, n, sp, la, lw), gq, a_w, y, att, ref, d = _i8_problem(ops, case, seed=11 + sum(map(ord, case)))
    geom = make_geom((n, c1, *sp), c2, 3, 1, 1)
    assert ops.conv_i8_out_supported(geom, la, lw)
    G = (a_w * (gq.float() / (lw - 1))).to(DEV)
    a = att if with_att else None
    atts = None if a is None else a.to(DEV)
    ptr = _poison((n, *sp, c2))
    out, sq = ops.conv_forward_i8(d["xidx"], G, d["b"], geom, d["y"], atts, d["alpha"], la, d["st"], lw)
    _check_poisoned(out, ptr)
    assert torch.equal(ops._keep_i8[0].reshape(gq.shape).cpu(), gq)      # the numerators, recovered from G / alpha
    scale = ref.abs().max().item()
    assert (_ncdhw(out).cpu().double() - ref).abs().max().item() <= 3e-7 * scale
    got = _i8_sums_vs_fp64(sq, ref, y, a)
    out2, sq2 = ops.conv_forward_i8(d["xidx"], G, d["b"], geom, d["y"], atts, d["alpha"], la, d["st"], lw)
    assert torch.equal(out2, out) and sq2.cpu().tolist() == got


def test_quantised_forward_rejects_a_mask_of_the_wrong_size(ops):
    """The kernel reads the mask at every output voxel: a batch-1 mask for a batch of 2 is refused on the host."""
    from efficientq_amd import _lib
    from efficientq_amd.hip_ops import make_geom
    n, c, sp, la, lw = 2, 32, (8, 4, 8), 4, 4
    geom = make_geom((n, c, *sp), c, 3, 1, 1)
    xidx = torch.zeros(n, *sp, c, dtype=torch.uint8, device=DEV)
    G = torch.full((c, c, 3, 3, 3), 0.05, device=DEV)
    y = torch.zeros(n, *sp, c, device=DEV)
    st = ops.new_fp_state()
    st[0] = 0.15
    alpha = torch.tensor(1.0, device=DEV)
    for bad in (torch.ones(1, *sp, device=DEV), torch.ones(n, *sp[:2], sp[2] + 1, device=DEV)):
        with pytest.raises(_lib.EffqError, match="att"):
            ops.conv_forward_i8(xidx, G, None, geom, y, bad, alpha, la, st, lw)


# ------------------------------------------------------------------ idle workgroups and the partial-sum slots
def test_idle_workgroups_overwrite_stale_partial_sums(ops):
    """A run in which every workgroup of the grid has a tile fills every partial-sum slot of the shared workspace with a
    non-zero value; the next run, on the same HipOps, has idle workgroups that must post zeros over those slots."""
    from efficientq_amd.hip_ops import make_geom
    gen = torch.Generator().manual_seed(21)

    def f32_loss(c1, sp, att):
        x = torch.relu(torch.randn(1, c1, *sp, generator=gen))
        w = torch.randn(32, c1, 3, 3, 3, generator=gen) * (1.0 / (27 * c1) ** 0.5)
        ref = F.conv3d(x.double(), w.double(), None, 1, 1)
        y = (ref + 0.1 * torch.randn(ref.shape, generator=gen).double()).float()
        a = torch.rand(1, *sp, generator=gen) + 0.5 if att else None
        _, sq = ops.conv_step(_ndhwc(x).to(DEV), w.to(DEV), None, make_geom(x.shape, 32, 3, 1, 1), _ndhwc(y).to(DEV),
                              None if a is None else a.to(DEV))
        return _sums_vs_fp64(sq, ref, y, a)

    # tiled k_conv3d_k3<1, *>: 512 tiles on a grid of 512, then 605 tiles with 209 idle workgroups
    assert f32_loss(32, (32, 32, 64), True)[0] > 0
    f32_loss(32, F32_CASES["k3_32to32"][6], True)
    # direct k_conv3d_c4h<1>: the same two tile counts
    assert f32_loss(4, (32, 32, 64), False)[0] > 0
    f32_loss(4, F32_CASES["first_4to32_s1"][6], False)

    # k_conv3d_i8w<false>: 256 tiles on a grid of 256, then 660 tiles with 36 idle workgroups
    for sp in ((16, 32, 64), I8_CASES["i8w_64to64"][3]):
        xidx = torch.randint(0, 4, (1, *sp, 64), generator=gen, dtype=torch.uint8)
        gq = (2 * torch.randint(0, 4, (64, 64, 3, 3, 3), generator=gen) - 3).to(torch.int8)
        y = torch.randn(1, *sp, 64, generator=gen)
        st = ops.new_fp_state()
        st[0] = 0.1
        ref = F.conv3d(xidx.permute(0, 4, 1, 2, 3).double(), gq.double(), None, 1, 1) * (0.5 * float(np.float32(0.1)) / 9)
        sq = torch.zeros(2, dtype=torch.float64, device=DEV)
        ops.conv_step_i8(xidx.to(DEV), gq.to(DEV), None, make_geom((1, 64, *sp), 64, 3, 1, 1), y.to(DEV),
                         torch.tensor(0.5, device=DEV), 4, st, 4, sq)
        assert _i8_sums_vs_fp64(sq, ref, y, None)[0] > 0
