"""The device pipeline of the `prep` mission on one synthetic subject (diagnostic, GPU), kernel by kernel, timed with HIP
events, one JSON line per subject.
--size brats: 4 x 240 x 240 x 155 float32, mask `nonzero` (a zero margin of 20 voxels per side);
--size lits:  1 x 512 x 512 x D (--depth, 300 by default) float32 HU-like values, mask `all`, window -200, 250, and the
  resampling from 0.8 x 0.8 x 2.5 mm to 1.6 mm (--factors d,h,w: other factors, e.g. 0.64,2,2 to down-sample along W),
  with the anti-alias filter of --prep_antialias ahead of it: `smooth` is the whole filter, `smooth_d`, `smooth_h`,
  `smooth_w` one filtered axis each (one pass: the volume read once and written once);
--size d,h,w with --modalities C: any other grid.
--factors d,h,w resamples any of them (brats: not resampled without it).  Beside `resample` (trilinear) the cubic
  B-spline path of --prep_interp cubic is timed: `resample_cubic` is the whole call (three prefilter passes and the
  evaluation), `spline_d`, `spline_h`, `spline_w` one prefilter pass each (d reads the float32 volume and writes the fp64
  coefficients, h and w filter them in place: read once and written once, 16 B per voxel), `cubic_eval` the rest.
`quantiles` is effq_prep_quantiles of --prep_window pLO,pHI on the source grid (p0.5, p99.5: R = 2; four passes over the
  subject, its bytes count the subject four times; the eight one-workgroup launches between and after them are in its
  time), `window_mask` the masked window of one modality; neither enters device_ms_total.
Each step runs once unmeasured, then REPS times (median), warm and after 512 MiB of other writes have pushed the subject
out of the Infinity Cache.  gbps = the bytes the step must move (what it reads once plus what it writes) over the time;
hbm_frac = that over the 8 TB/s peak.  numpy_ms is the same arithmetic on the host in numpy, one run, as context."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from efficientq_amd import prep
from efficientq_amd.hip_ops import get_ops

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="brats")
ap.add_argument("--depth", type=int, default=300)
ap.add_argument("--modalities", type=int, default=1)
ap.add_argument("--no_numpy", action="store_true")
ap.add_argument("--factors", default=None)
cli = ap.parse_args()
REPS = int(os.environ.get("REPS", "7"))
HBM_PEAK = 8.0e12
dev = "cuda:0"
ops = get_ops(dev)
g = torch.Generator().manual_seed(0)

if cli.size == "brats":
    C, grid, mask, window, factors = 4, (240, 240, 155), "nonzero", None, None
elif cli.size == "lits":
    C, grid, mask, window, factors = 1, (512, 512, cli.depth), "all", (-200.0, 250.0), (2.0, 2.0, 0.64)
else:
    C, grid, mask, window, factors = cli.modalities, tuple(int(v) for v in cli.size.split(",")), "nonzero", None, None
if cli.factors:
    factors = tuple(float(v) for v in cli.factors.split(","))
S = grid[0] * grid[1] * grid[2]
x = torch.randn(C, *grid, generator=g) * 300.0 + 40.0
if mask == "nonzero":
    body = torch.zeros(grid, dtype=torch.bool)
    body[20:-20, 20:-20, 20:-20] = True
    x = x * body
x = x.to(dev).contiguous()
evict = torch.empty(512 << 20, dtype=torch.uint8, device=dev)


def timed(fn, before=None):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


res = {"size": cli.size, "modalities": C, "grid": list(grid), "mask": mask}


def step(name, fn, nbytes):
    ms, cold = timed(fn), timed(fn, before=lambda: evict.fill_(1))
    res[name] = {"ms": round(ms, 4), "ms_after_evict": round(cold, 4), "bytes": nbytes,
                 "gbps": round(nbytes / (ms * 1e-3) / 1e9, 1), "gbps_after_evict": round(nbytes / (cold * 1e-3) / 1e9, 1),
                 "hbm_frac_after_evict": round(nbytes / (cold * 1e-3) / HBM_PEAK, 3)}


step("quantiles", lambda: ops.prep_quantiles(x.reshape(C, -1), (0.5, 99.5), mask), 4 * 4 * C * S)
res["quantiles"]["passes"] = 4
plane = x[0].clone()
step("window_mask", lambda: ops.prep_window_mask(plane, -1e30, 1e30, mask), 2 * 4 * S)
del plane
if window is not None:
    step("window", lambda: ops.prep_window(x, *window), 2 * 4 * C * S)
if factors is not None:
    out = tuple(prep.resample_extent(n, f) for n, f in zip(grid, factors))
    # --prep_antialias: the whole filter, then each filtered axis alone (one pass: the volume read once, written once)
    sig = tuple(prep.antialias_sigma(f) if prep.antialias_radius(prep.antialias_sigma(f)) else 0.0 for f in factors)
    axes = [a for a in range(3) if sig[a] > 0]
    if axes:
        step("smooth", lambda: ops.prep_smooth(x, sig, mask == "nonzero"), len(axes) * 2 * 4 * C * S)
        res["smooth"]["sigmas"], res["smooth"]["radii"] = list(sig), [prep.antialias_radius(s) for s in sig]
        for a in axes:
            one = tuple(sig[b] if b == a else 0.0 for b in range(3))
            step("smooth_" + "dhw"[a], lambda: ops.prep_smooth(x, one, mask == "nonzero"), 2 * 4 * C * S)
    step("resample", lambda: ops.prep_resample(x, factors, out), 4 * C * (S + out[0] * out[1] * out[2]))
    # --prep_interp cubic: the whole call, then its prefilter passes one by one; the evaluation is the difference
    O = out[0] * out[1] * out[2]
    step("resample_cubic", lambda: ops.prep_resample_cubic(x, factors, out, mask == "nonzero"),
         C * (4 * S + 8 * S + 2 * 16 * S + 8 * S + 4 * O))
    coef = ops.prep_spline_prefilter(x, "d")
    step("spline_d", lambda: ops.prep_spline_prefilter(x, "d", out=coef), C * (4 + 8) * S)
    for a in "hw":
        step("spline_" + a, lambda: ops.prep_spline_prefilter(x, a, out=coef), C * 16 * S)      # in place, again and again
    res["cubic_eval"] = {"ms": round(res["resample_cubic"]["ms"] - sum(res["spline_" + a]["ms"] for a in "dhw"), 4),
                         "bytes": C * (8 * S + 4 * O)}
    del coef
    x = ops.prep_resample(x, factors, out)
    grid, S = out, out[0] * out[1] * out[2]
    res["resampled_grid"] = list(grid)
step("bbox_moments", lambda: ops.prep_bbox_moments(x, mask), 4 * C * S)
bbox, count, total = (t.cpu().tolist() for t in ops.prep_bbox_moments(x, mask))
mean = [s / n for s, n in zip(total, count)]
step("sqdev", lambda: ops.prep_sqdev(x, mean, mask), 4 * C * S)
std = [float(np.sqrt(q / n)) for q, n in zip(ops.prep_sqdev(x, mean, mask).cpu().tolist(), count)]
pmin, pmax = tuple(bbox[:3]), tuple(b + 1 for b in bbox[3:])
crop = (pmax[0] - pmin[0]) * (pmax[1] - pmin[1]) * (pmax[2] - pmin[2])
step("standardise_crop", lambda: ops.prep_standardise_crop(x, pmin, pmax, mean, std, mask), 2 * 4 * C * crop)
res["crop"] = [list(pmin), list(pmax)]
res["device_ms_total"] = round(sum(v["ms"] for k, v in res.items()
                                   if isinstance(v, dict) and not k.startswith(("smooth_", "spline_", "cubic_")) and
                                   k not in ("resample_cubic", "quantiles", "window_mask")), 3)      # the trilinear pipeline; `smooth` holds its passes

if not cli.no_numpy:
    h = x.cpu().numpy()
    t0 = time.perf_counter()
    m = np.ones(h.shape, bool) if mask == "all" else h != 0
    idx = np.nonzero(m.any(0))
    lo, hi = [int(i.min()) for i in idx], [int(i.max()) + 1 for i in idx]
    y = np.zeros((C, hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]), np.float32)
    for c in range(C):
        v = h[c][m[c]].astype(np.float64)
        mu = v.mean()
        sd = np.sqrt(((v - mu) ** 2).mean())
        box = (slice(lo[0], hi[0]), slice(lo[1], hi[1]), slice(lo[2], hi[2]))
        y[c] = np.where(m[c][box], ((h[c][box].astype(np.float64) - mu) / sd).astype(np.float32), np.float32(0))
    res["numpy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
print(json.dumps(res))
