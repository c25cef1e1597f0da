"""effq_fixed_point_traj (csrc/fixed_point_traj.hip, csrc/fp_traj.h, the recorder of csrc/fp_level.h) restated in fp64 numpy
(tests/test_fp_traj_ref_cpu.py, tests/test_fp_traj_classes_gpu.py).  No GPU, no library; the three reductions of the loop
are torch's fp64 sums, the oracle's, so that the restatement can be pinned to it bit for bit.

  iterates  the loop of project_by_iter (layer_helper.py:40-70) as oracle.effq_oracle.fit_scale runs it, keeping every
            classification scale and how far each stop decision was from the tolerance;
  classify  what phase 1 does with a prediction: the bracket ends, which values it lists, and which of the three ways
            (narrow list / both lists / full pass) phase 2 serves every iterate;
  record    what the recorder leaves in the prediction for the next call.

The constants of the recorder are literals here on purpose: a retuned header then fails the tests instead of being
followed by them."""
import math

import numpy as np
import torch

SLOTS = 8                        # FPT_SLOTS
WGV = 4096                       # values a workgroup takes (FPT_T * FPT_EPT)
ONE_WAVE_MAX = 1024              # narrow list served from the first wave's registers (64 * FPT_FC)
REGISTER_MAX = 4096              # ... from the workgroup's registers (FPT_CR * FPT_T); longer lists are streamed
MAXN = 1 << 23


def clustered(n, seed, alpha=0.07, spread=0.15):
    """Weights as the ADMM loop sees them: clustered around the four levels of a scale (fp32)."""
    rng = np.random.default_rng(seed)
    lv = np.array([-1.0, -1.0 / 3.0, 1.0 / 3.0, 1.0])[rng.integers(0, 4, n)]
    return (alpha * (lv + spread * rng.standard_normal(n))).astype(np.float32)


def normal(n, seed, sigma=0.05):
    return (sigma * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


# the seven calls that reach every way phase 2 serves an iterate (factors on one tensor): cold; inside the new 1 % margins;
# a drift of 1e-5 (the margins shrink to 0.85 % and 1e-4); 5.9e-4 (past the narrow margin: both lists); 8 % (past the wide
# one: full passes of a warm call; the margins go to their cap); 1e-4; 0 (a narrow margin of 2.5e-4)
SCHEDULE = (1.0, 1.002, 1.00201, 1.0026, 1.0026 * 1.08, 1.0026 * 1.08 * 1.0001, 1.0026 * 1.08 * 1.0001)


def scheduled(base, k):
    """The tensor of call k of SCHEDULE: the product in fp64, rounded once to fp32."""
    return (np.asarray(base, dtype=np.float64) * SCHEDULE[k]).astype(np.float32)


def level_exact(x, a, lo, hi, d):
    """level_exact of csrc/fp_level.h: C's fmin / fmax drop a NaN operand."""
    with np.errstate(all="ignore"):
        t = np.asarray(x, dtype=np.float64) / float(a)
        t = np.fmin(np.fmax(t, lo), hi)
        return np.rint((t - lo) / d)


def _sum(a):
    """The oracle's reduction (torch's fp64 sum over a contiguous vector): iterates is pinned to fit_scale to the last
    bit, which numpy's pairwise order misses by an ulp at 16 levels."""
    return float(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).sum())


def iterates(v, levels, lo, hi, tol, max_iter):
    """dict(alphas = the classification scales alpha_0 .. alpha_{it-1}, alpha = the final scale, it, done, stop_margin,
    sum_abs).  done = 2 whenever it == max_iter (fp_stop: the reference raises at the cap even if the last step
    converged) and where a scale is not a positive finite number (the kernels stop there; the reference would spin)."""
    x = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    d = (hi - lo) / (levels - 1)
    sum_abs = _sum(np.abs(x))
    a, alphas, it, done, margin = float(torch.from_numpy(x).abs().mean()), [], 0, 0, math.inf
    while not done:
        if not (a > 0.0) or not (a < 1e300):
            done = 2
            break
        alphas.append(a)
        b = level_exact(x, a, lo, hi, d) * d + lo
        with np.errstate(all="ignore"):
            a_new = _sum(b * x) / _sum(b * b)
        it += 1
        step = abs(a_new - a)
        if not math.isnan(step):
            margin = min(margin, abs(step - tol))
        if it >= max_iter:
            done = 2
        elif not (step > tol):
            done = 1
        a = a_new
    return {"alphas": alphas, "alpha": a, "it": it, "done": done, "stop_margin": margin, "sum_abs": sum_abs}


def bracket_ends(pred):
    """(K, warm, ends[K][4]): wide lo, narrow lo, narrow hi, wide hi of every valid slot, as fpt_phase1 forms them."""
    K = min(max(int(pred["K"]), 0), SLOTS)
    warm = K > 0 and int(pred["e_valid"]) != 0
    ends = np.zeros((K, 4))
    with np.errstate(all="ignore"):
        for j in range(K):
            ew = np.float64(pred["eps"][j])
            en = np.fmin(np.float64(pred["eps_n"][j]), ew)
            l, h = np.float64(pred["lo"][j]), np.float64(pred["hi"][j])
            e = (l * (1.0 - ew), l * (1.0 - en), h * (1.0 + en), h * (1.0 + ew))
            # a slot that is not positive and ordered (no record of a call) is dead: no scale is inside NaN ends
            ends[j] = e if (e[0] > 0.0 and e[0] <= e[1] <= e[2] <= e[3] < 1e300) else (math.nan,) * 4
    return K, warm, ends


def classify(pred, v, levels, lo, hi, alphas=()):
    """Phase 1 on the prediction fields `pred` (K, lo, hi, eps, eps_n, e, e_valid as read from the device before the call)
    and, for every iterate of `alphas`, the way phase 2 serves it: 'n' from the narrow list, 'r' from both lists, 'f' by
    a full pass.  dict(m_n, m_r, tallies_ok, classes, bracket_margin, K, warm)."""
    x = np.ascontiguousarray(v, dtype=np.float32).reshape(-1).astype(np.float64)
    d = (hi - lo) / (levels - 1)
    K, warm, ends = bracket_ends(pred)
    m_n = m_r = 0
    if warm:
        with np.errstate(all="ignore"):
            h_lo, h_hi = np.fmin.reduce(ends[:, 0]), np.fmax.reduce(ends[:, 3])
        cross = level_exact(x, h_lo, lo, hi, d) != level_exact(x, h_hi, lo, hi, d)
        w = x[cross]                               # the worklist: the level changes somewhere inside the hull
        narrow, ring = np.zeros(w.size, dtype=bool), np.zeros(w.size, dtype=bool)
        for j in range(K):
            wide_ne = level_exact(w, ends[j, 0], lo, hi, d) != level_exact(w, ends[j, 3], lo, hi, d)
            narrow_ne = level_exact(w, ends[j, 1], lo, hi, d) != level_exact(w, ends[j, 2], lo, hi, d)
            narrow |= wide_ne & narrow_ne
            ring |= wide_ne & ~narrow_ne
        m_n = int(np.count_nonzero(narrow))
        m_r = int(np.count_nonzero(ring & ~narrow))
    sum_abs = float(np.abs(x).sum())
    bound = (levels - 1) * sum_abs
    e_full = 58 - (math.frexp(bound)[1] - 1) if 0.0 < bound < 1e300 else 0
    e = max(min(int(pred["e"]), 2000), -2000)
    tallies_ok = bool(warm and bound * math.ldexp(1.0, min(e, 900)) < 2.0e18 and e_full - 2 <= e <= e_full + 2)
    classes, margin = [], math.inf
    for i, a in enumerate(alphas):
        if not tallies_ok:
            classes.append("f")
            continue
        j = min(i, K - 1)
        e = ends[j]
        in_w = bool(a >= e[0] and a <= e[3])
        in_n = bool(in_w and a >= e[1] and a <= e[2])
        classes.append("n" if in_n else "r" if in_w else "f")
        with np.errstate(all="ignore"):
            m = np.abs(a - e) / a
        margin = min(margin, float(np.nanmin(m)) if not np.all(np.isnan(m)) else math.inf)
    return {"m_n": m_n, "m_r": m_r, "tallies_ok": tallies_ok, "classes": "".join(classes), "bracket_margin": margin,
            "K": K, "warm": warm}


def record(pred, alphas, alpha, sum_abs, levels):
    """The prediction fields after a call that classified at `alphas` and ended at `alpha` (fpt_note, fpt_finish_slot,
    fpt_finish_head): dict(K, lo, hi, eps, eps_n, e, e_valid).  Slots beyond the new K keep what they held."""
    it = len(alphas)
    nlo, nhi = [0.0] * SLOTS, [0.0] * SLOTS
    for i, a in enumerate(alphas):
        if i < SLOTS:
            nlo[i] = nhi[i] = a
        else:
            nlo[SLOTS - 1], nhi[SLOTS - 1] = min(nlo[SLOTS - 1], a), max(nhi[SLOTS - 1], a)
    K_old, K = int(pred["K"]), min(it, SLOTS)
    out = {k: list(pred[k]) for k in ("lo", "hi", "eps", "eps_n")}
    for j in range(K):
        l, h = nlo[j], nhi[j]
        if j == K - 1:
            l, h = min(l, alpha), max(h, alpha)
        eps = eps_n = 0.01
        if j < K_old and K_old <= SLOTS:
            drift = max(abs(l - pred["lo"][j]), abs(h - pred["hi"][j])) / abs(h)
            eps = min(max(max(4.0 * drift, 0.85 * pred["eps"][j]), 1e-4), 0.03)
            eps_n = min(max(2.5 * drift, 1e-4), eps)
        out["lo"][j], out["hi"][j], out["eps"][j], out["eps_n"][j] = l, h, eps, eps_n
    bound = (levels - 1) * float(sum_abs)
    ok = bound > 0.0 and bound < 1e300
    out.update(K=K, e=(58 - (math.frexp(bound)[1] - 1)) if ok else 0, e_valid=1 if ok else 0)
    return out


def cold_pred():
    """The fields of a zero-filled prediction: nothing known."""
    z = [0.0] * SLOTS
    return {"K": 0, "e": 0, "e_valid": 0, "lo": list(z), "hi": list(z), "eps": list(z), "eps_n": list(z)}


def ulp_shift(x, k):
    """The fp32 values k units in the last place above (k < 0: below) x."""
    i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    m = np.where(i >= 0, i, -(i & 0x7FFFFFFF)) + int(k)
    return np.where(m >= 0, m, (-m) | 0x80000000).astype(np.uint32).view(np.float32)


def adversarial(levels, seed=1234, lo=-1.0, hi=1.0, tol=1e-5):
    """The constructions of test_bucketed_fixed_point_on_adversarial_values as {name: fp32 vector of ~20 000}: values ON
    the level boundaries (k - 0.5) d + lo of EVERY iterate of the base tensor's fixed point and one ulp either side (a
    value whose level differs between the two ends of any bracket around that iterate, however narrow), signed zeros
    and denormals, duplicates, one heavy outlier, an all-equal tensor, two values."""
    rng = np.random.default_rng(seed + levels)
    base = (0.1 * rng.standard_normal(20000)).astype(np.float32)
    fit = iterates(base, levels, lo, hi, tol, 100 * levels)
    d = (hi - lo) / (levels - 1)
    bnd = (np.arange(1, levels) - 0.5) * d + lo
    p = np.concatenate([(bnd * a).astype(np.float32) for a in fit["alphas"] + [fit["alpha"]]])
    pts = np.concatenate([p, ulp_shift(p, 1), ulp_shift(p, -1)])
    f32 = np.float32
    out = base.copy()
    out[0] = 500.0
    return {
        "boundaries": np.concatenate([base] + [pts] * max(1, min(7, 4000 // pts.size))),
        "zeros_tiny": np.concatenate([base, np.zeros(500, f32), -np.zeros(300, f32), np.full(200, -1e-30, f32),
                                      np.full(200, 1e-30, f32), np.full(100, -1e-42, f32)]),
        "duplicates": (np.round(base.astype(np.float64) * 50) / 50).astype(f32),
        "outlier": out,
        "all_equal": np.full(20000, 0.37, f32),
        "two_values": np.concatenate([np.full(12000, -0.2, f32), np.full(8000, 0.9, f32)]),
    }


# (n, levels, tensor) of the seven-call schedule.  4 levels on the clustered tensor: the three lengths of the narrow list;
# 3 levels on a normal one: 9 iterations, the tail slot in use; 16 levels: ~60 iterations, narrow, ring and full inside one
# call; 2 levels (one more case than the issue lists: none of the others has a K = 1 call): one iteration, empty lists
SCHEDULE_CASES = ((4095, 4, "clustered"), (65541, 4, "clustered"), (262149, 4, "clustered"), (65541, 3, "normal"),
                  (65541, 16, "normal"), (65541, 2, "normal"))
REQUIRED = ("m_n <= 1024", "1024 < m_n <= 4096", "m_n > 4096", "ring iterate", "full iterate of a warm call",
            "iterates beyond slot 7", "K = 1 call")


def schedule_base(n, levels, kind):
    return clustered(n, 3 * n + levels) if kind == "clustered" else normal(n, 3 * n + levels)


def reached(cls, n_iterates):
    """Which of REQUIRED one call reaches, from its classify result."""
    got = set()
    if cls["tallies_ok"]:
        if "n" in cls["classes"] or "r" in cls["classes"]:          # (a list that no iterate scans pins nothing)
            got.add("m_n <= 1024" if cls["m_n"] <= ONE_WAVE_MAX else
                    "1024 < m_n <= 4096" if cls["m_n"] <= REGISTER_MAX else "m_n > 4096")
        if "r" in cls["classes"]:
            got.add("ring iterate")
        if "f" in cls["classes"]:
            got.add("full iterate of a warm call")
        if n_iterates > SLOTS and cls["classes"][SLOTS:].strip("f"):
            got.add("iterates beyond slot 7")
        if cls["K"] == 1:
            got.add("K = 1 call")
    return got
