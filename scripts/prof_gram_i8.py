"""Time effq_gram_accum_i8 on the BraTS layer shapes: python scripts/prof_gram_i8.py [N] [--f32] [--small].

Per shape it prints the launch (pairs, groups, splits), the bytes one launch stages into LDS and the rate that makes of
the measured time.  With a library that has effq_gram_i8_set_group the default grouping and one pair per workgroup are
timed side by side and their outputs compared bit for bit.  On an ablation build (make ABLATE=1), started with
EFFQ_GI8_DEBUG=0 in the environment, every row is repeated with EFFQ_GI8_DEBUG = 1, 2, 3 (no MFMA and with it no flush,
every global load from one address, no LDS staging); the library reads the variable at every launch.  --f32 also times
the fp32 Gram, --small adds the 1^3 layers."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from efficientq_amd.hip_ops import get_ops, make_geom
dev = "cuda:0"; ops = get_ops(dev)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 16
shapes = [(32, 32, 64, 3), (64, 64, 32, 3), (128, 128, 16, 3), (256, 256, 8, 3)]
if "--small" in sys.argv:
    shapes += [(128, 64, 16, 1), (128, 256, 8, 1), (256, 128, 8, 1), (64, 32, 32, 1)]
has_groups = hasattr(ops, "gram_i8_groups")
groupings = ((0, 0), (1, 1)) if has_groups else ((0, 0),)
ablations = (0, 1, 2, 3) if os.environ.get("EFFQ_GI8_DEBUG") is not None else (0,)


def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for C, C2, S, K in shapes:
    g = torch.Generator(device=dev).manual_seed(C)
    idx = torch.randint(0, 4, (N, S, S, S, C), generator=g, device=dev).to(torch.uint8)
    alpha = torch.tensor(0.8, device=dev)
    y = torch.randn(N, S, S, S, C2, generator=g, device=dev)
    att = torch.randint(1, 3, (N, S, S, S), generator=g, device=dev).float()
    geom = make_geom((N, C, S, S, S), C2, K, 1, K // 2)
    cls = ops.att_classes(att)
    n = C * K ** 3 + 1; V = N * S ** 3
    ops_n = 2.0 * n * n * V + 2.0 * C2 * n * V
    plan = ops.gram_i8_plan(geom, cls[3], cls[0].numel())
    outs = {}
    for grp in groupings:
        if has_groups:
            ops.gram_i8_set_group(*grp)
            gq = ops.gram_i8_groups(geom, cls[3], cls[0].numel())
        else:
            gq = dict(gi=1, gj=1, ngroups=plan["npairs"], grid_y=plan["nsplit"])
        # one workgroup stages (gi + gj) * 128 rows x 128 voxels per chunk (a diagonal group: gi * 128 rows)
        nb, nbx, G = plan["NB"], plan["NBX"], gq["gi"]
        ndiag = (nbx + G - 1) // G
        staged = ((gq["ngroups"] - ndiag) * 2 * G + ndiag * G) * 128 * 128 * plan["nchunks"]
        for dbg in ablations:
            if len(ablations) > 1:
                os.environ["EFFQ_GI8_DEBUG"] = str(dbg)
            fn = lambda: ops.gram_i8(idx, cls, y, geom, True, alpha, 4, unweighted=True)
            ms = timed(fn)
            if dbg == 0:
                outs[grp] = fn()
            print(f"gram i8  C={C}->{C2} k={K} n={n} V={V} pairs={plan['npairs']} group={G}x{G} groups={gq['ngroups']} "
                  f"splits={gq['grid_y']} debug={dbg}: {ms:8.3f} ms  {ops_n / ms / 1e9:8.1f} TOP/s algorithmic  "
                  f"staged {staged / 1e9:6.2f} GB = {staged / ms / 1e9:6.2f} TB/s", flush=True)
    if has_groups:
        ops.gram_i8_set_group(0, 0)
        same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs[(0, 0)], outs[(1, 1)]))
        print(f"         default grouping and 1x1 bit-identical: {same}", flush=True)
        assert same
    if "--f32" in sys.argv:
        xhat = (idx.float() * (alpha / 3)).contiguous()
        ms = timed(lambda: ops.gram(xhat, att, y, geom, True), 3)
        print(f"gram f32 C={C}->{C2} k={K} n={n} V={V}: {ms:8.3f} ms  {ops_n / ms / 1e9:8.1f} TFLOP/s algorithmic", flush=True)
