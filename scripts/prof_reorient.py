"""effq_prep_reorient on one LiTS-sized volume (diagnostic, GPU): both variants against a device-to-device copy of the
same bytes, timed with HIP events, one JSON line.
--size d,h,w (384,512,512 by default), float32 and uint8.  Per element size: `copy` (torch's copy_ of the volume into a
second buffer: the yardstick), `rows` (variant 0: src_axis 0,1,2 with the innermost axis reversed), `rows_swap` (variant
0: D and H exchanged), `tile_hw` (variant 1: H and W exchanged), `tile_dw` (variant 1: D and W exchanged, D and W
reversed), `tile_rot` (variant 1: src_axis 1,2,0).  The arms alternate inside one loop of REPS rounds after WARM unmeasured
rounds, each round times every arm once over INNER back-to-back launches; ms = the median over the rounds of the time per
launch, lo / hi = the least and the greatest round.  The volume and its copy are 2 x 384 MiB (float32) or 2 x 96 MiB (uint8):
the float32 arms run from HBM, the uint8 ones fit the 256 MiB Infinity Cache, so EVICT=1 writes 512 MiB elsewhere before
every launch of a round (INNER is then 1).  gbps = (bytes read + bytes written) / time; vs_copy = the arm's rate over the
copy's.  Every arm's result is compared once, in full, with torch's own permute and flip."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from efficientq_amd.hip_ops import get_ops

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="384,512,512")
cli = ap.parse_args()
REPS, WARM = int(os.environ.get("REPS", "9")), int(os.environ.get("WARM", "2"))
EVICT = os.environ.get("EVICT", "0") == "1"
INNER = 1 if EVICT else int(os.environ.get("INNER", "10"))
dev = "cuda:0"
ops = get_ops(dev)
shape = (1,) + tuple(int(v) for v in cli.size.split(","))
ARMS = {"rows": ((0, 1, 2), (False, False, True)), "rows_swap": ((1, 0, 2), (False, False, False)),
        "tile_hw": ((0, 2, 1), (False, False, False)), "tile_dw": ((2, 1, 0), (True, False, True)),
        "tile_rot": ((1, 2, 0), (False, False, False))}
evict = torch.empty(512 << 20, dtype=torch.uint8, device=dev) if EVICT else None
res = {"size": list(shape[1:]), "reps": REPS, "inner": INNER, "evict": EVICT}

for dtype in (torch.float32, torch.uint8):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randint(0, 255, shape, generator=g, device=dev, dtype=torch.uint8).to(dtype)
    other = torch.empty_like(x)
    nbytes = 2 * x.numel() * x.element_size()
    fns = {"copy": lambda: other.copy_(x)}
    for name, (axes, flip) in ARMS.items():
        want = x.permute(0, *(1 + a for a in axes))
        if any(flip):
            want = want.flip([1 + p for p in range(3) if flip[p]])
        assert torch.equal(ops.prep_reorient(x, axes, flip), want), name
        assert ops.prep_reorient_variant(axes, flip, x.element_size()) == (0 if name.startswith("rows") else 1)
        del want
        fns[name] = (lambda a, f: lambda: ops.prep_reorient(x, a, f))(axes, flip)
    times = {k: [] for k in fns}
    for r in range(WARM + REPS):
        for name, fn in fns.items():
            if EVICT:
                evict.fill_(r)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(INNER):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r >= WARM:
                times[name].append(a.elapsed_time(b) / INNER)
    out = {}
    for name, ms in times.items():
        ms = sorted(ms)
        med = ms[len(ms) // 2]
        out[name] = {"ms": round(med, 4), "lo": round(ms[0], 4), "hi": round(ms[-1], 4),
                     "gbps": round(nbytes / (med * 1e-3) / 1e9, 1)}
    for name in out:
        out[name]["vs_copy"] = round(out[name]["gbps"] / out["copy"]["gbps"], 3)
    res[str(dtype).replace("torch.", "")] = out
print(json.dumps(res))
