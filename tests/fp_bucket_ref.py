"""The dispatch of effq_fixed_point_bucket_rec (csrc/fixed_point_bucket.hip) restated in numpy (tests/test_fp_bucket_ref_cpu.py,
tests/test_fp_bucket_classes_gpu.py).  No GPU, no library.  The fixed point itself, the level function, the recorder and the
adversarial constructions are fp_traj_ref's; this file adds what is the bucketed kernel's own:

  geometry          which path a tensor takes (k_fps<8 / 16 / 32> in one workgroup, or the four launches), the bucket function
                    in the kernel's fp32 arithmetic, the finer integer unit of k_fps on a range an outlier stretched;
  classes           for every classification scale and every level boundary the guard band, the boundary segment and what
                    the iteration phase has to do with it, tallied by class;
  counts_by_rule /  the below-counts per iterate and boundary by the kernel's rule (v <= band's lower end, the reference's
  counts_direct     arithmetic inside the band) and by level_exact < k over all values;
  workspace_layout  the byte ranges of fpg_carve;
  CASES             the table the GPU module runs, with the classes each row is there for.

The order of the values INSIDE a bucket is whatever the atomics of the build passes made it, so where a class depends on the
position of a value in its segment (cached or not, which lane sums it) the tallies count only what holds in EVERY order.

The constants are literals on purpose: a retuned kernel then fails the tests instead of being followed by them."""
import collections
import functools
import math

import numpy as np

from tests import fp_traj_ref as R

B_S, B_G = 2048, 8192            # buckets of the one-workgroup path / of the four launches
S_MAXN = 32768                   # values the one-workgroup path takes
S_T = 1024                       # its threads: k_fps<PER> holds ceil(n / 1024) <= PER values per thread
TI = 256                         # threads of the iteration phase
CR = 4                           # boundary-segment values cached per lane
SHIFT = 36                       # integer unit = bucket width * 2^-36
MAXN = 1 << 23
SUM_WG = 2048                    # values per workgroup of the sum and scatter kernels
SLICE = 8192                     # values per workgroup of the count kernel
MAXBLK = 4096                    # sum workgroups the partials array has room for
MAXB = 65536                     # buckets the workspace tables have room for
TOL = 1e-5

f32 = np.float32


def fpb_step(v, direction):
    """fpb_step: one fp32 step down / up on the ordered key of the value, saturating at -+FLT_MAX.  (Not ulp_shift: that
    one takes both zeros for one value; the kernel steps from +0 to -0.)"""
    u = np.ascontiguousarray(v, dtype=f32).view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    if direction < 0:
        key = np.where(key > 0x00800000, key - 1, 0x00800000)
    else:
        key = np.where(key < 0xFF7FFFFF, key + 1, 0xFF7FFFFF)
    u = np.where(key & 0x80000000, key & 0x7FFFFFFF, ~key & 0xFFFFFFFF)
    return u.astype(np.uint32).view(f32)


def gs_of(levels):
    """Lanes per boundary of the iteration phase."""
    p2 = 1
    while p2 < levels - 1:
        p2 <<= 1
    return max(1, min(64, TI // p2))


class Geometry:
    def __init__(self, v):
        x = np.ascontiguousarray(v, dtype=f32).reshape(-1)
        self.n = n = x.size
        self.path = "S" if n <= S_MAXN else "G"
        per = -(-n // S_T)
        self.inst = (8 if per <= 8 else 16 if per <= 16 else 32) if self.path == "S" else None
        self.B = B_S if self.path == "S" else B_G
        with np.errstate(all="ignore"):
            mx = np.fmax.reduce(np.abs(x)) if n else f32(0)                   # fmaxf drops a NaN
            self.sum_abs = R._sum(np.abs(x.astype(np.float64)))
            self.ratio = float(mx) * n / self.sum_abs if self.sum_abs > 0 else math.nan
        self.extra = 0
        if self.path == "S" and 64.0 <= self.ratio < 1e30:
            self.extra = min((math.frexp(self.ratio)[1] - 1) - 5, 7)             # ilogb(ratio) - 5
        r = f32(mx)
        if not r >= f32(1e-30):
            r = f32(1e-30)
        if not r <= f32(3.0e38):
            r = f32(3.0e38)
        self.R = r
        with np.errstate(all="ignore"):
            self.scale = f32(self.B) / (f32(2.0) * r)                           # fp32, as fpb_geo
        self.R64 = float(r)
        self.w = 2.0 * self.R64 / self.B
        self.q = math.ldexp(self.w, -(SHIFT + self.extra))                      # the integer unit
        self.sum_blocks = -(-n // SUM_WG) if self.path == "G" else 0
        self.count_slices = -(-n // SLICE) if self.path == "G" else 0

    def bucket(self, v):
        """fpb_bucket in fp32: clamp(floor((v + R) * scale), 0, B - 1)."""
        with np.errstate(all="ignore"):
            f = np.floor((np.asarray(v, dtype=f32) + self.R) * self.scale)
            f = np.fmin(np.fmax(f, f32(0)), f32(self.B - 1))
        return f.astype(np.int64)

    def origin(self, j):
        """What the integer units of a segment that starts at bucket j count from: the lower edge of bucket j - 1."""
        return (np.asarray(j, dtype=np.float64) - 1.0) * self.w - self.R64


def geometry(v):
    return Geometry(v)


def _bands(g, levels, lo, hi, a):
    """The guard bands of every boundary k = 1 .. L-1 at scale a: (vlo, vhi, jlo, jhi)."""
    d = (hi - lo) / (levels - 1)
    kpos = lo + (np.arange(1, levels, dtype=np.float64) - 0.5) * d
    tk = a * kpos
    guard = np.maximum(np.abs(tk) * 2.0 ** -20, a * 2.0 ** -30)
    with np.errstate(all="ignore"):
        vlo, vhi = fpb_step((tk - guard).astype(f32), -1), fpb_step((tk + guard).astype(f32), +1)
    return vlo, vhi, g.bucket(vlo), g.bucket(vhi)


class _Sorted:
    """The tensor as the iteration phase sees it: grouped by bucket (here: sorted, which groups it too)."""

    def __init__(self, v):
        self.x = np.ascontiguousarray(v, dtype=f32).reshape(-1)
        self.g = Geometry(self.x)
        self.xs = np.sort(self.x)
        self.bk = self.g.bucket(self.xs)
        assert np.all(np.diff(self.bk) >= 0), "the bucket function is not monotone"
        self.csum = np.concatenate([[0.0], np.cumsum(self.xs.astype(np.float64))])

    def cnt_below(self, j):
        return np.searchsorted(self.bk, j, side="left")


def _fit(v, levels, lo, hi, tol, max_iter):
    return R.iterates(v, levels, lo, hi, tol, 100 * levels if max_iter is None else max_iter)


def _in_band_below(s, levels, lo, hi, a, i_lo, i_hi):
    """Per boundary: how many of the values strictly inside its band the reference's arithmetic puts below it."""
    d = (hi - lo) / (levels - 1)
    out = np.zeros(levels - 1, dtype=np.int64)
    for ki in np.nonzero(i_hi > i_lo)[0]:
        lv = R.level_exact(s.xs[i_lo[ki]:i_hi[ki]], a, lo, hi, d)
        out[ki] = np.count_nonzero(lv < ki + 1)
    return out


def counts_by_rule(v, levels, lo, hi, tol=TOL, max_iter=None, fit=None):
    """[iterate][k - 1]: values below boundary k as the kernel counts them."""
    s = _Sorted(v)
    fit = fit or _fit(s.x, levels, lo, hi, tol, max_iter)
    out = np.zeros((len(fit["alphas"]), levels - 1), dtype=np.int64)
    for i, a in enumerate(fit["alphas"]):
        vlo, vhi, _, _ = _bands(s.g, levels, lo, hi, a)
        i_lo, i_hi = np.searchsorted(s.xs, vlo, side="right"), np.searchsorted(s.xs, vhi, side="left")
        i_hi = np.maximum(i_hi, i_lo)
        out[i] = i_lo + _in_band_below(s, levels, lo, hi, a, i_lo, i_hi)
    return out


def level_counts(v, levels, lo, hi, a):
    """How many values the reference puts on each level at scale a."""
    d = (hi - lo) / (levels - 1)
    lv = R.level_exact(np.ascontiguousarray(v, dtype=f32).reshape(-1), a, lo, hi, d).astype(np.int64)
    return np.bincount(lv, minlength=levels)


def counts_direct(v, levels, lo, hi, tol=TOL, max_iter=None, fit=None):
    """[iterate][k - 1]: values with level_exact < k."""
    fit = fit or _fit(v, levels, lo, hi, tol, max_iter)
    out = np.zeros((len(fit["alphas"]), levels - 1), dtype=np.int64)
    for i, a in enumerate(fit["alphas"]):
        out[i] = np.cumsum(level_counts(v, levels, lo, hi, a))[:-1]
    return out


def sum_bb(counts, levels, lo, hi):
    """sum_m b_m^2 C_m from the level counts, in extended precision: what the kernel's fp64 sum is held to."""
    d = np.longdouble(hi - lo) / np.longdouble(levels - 1)
    d = np.longdouble(float(d))                                             # (the kernel's d is an fp64 number)
    bm = np.arange(levels, dtype=np.longdouble) * d + np.longdouble(lo)
    return float(np.sum(bm * bm * counts.astype(np.longdouble)))


def sum_bv(v, levels, lo, hi, a):
    """The reference's sum b v at scale a."""
    x = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    d = (hi - lo) / (levels - 1)
    return R._sum((R.level_exact(x, a, lo, hi, d) * d + lo) * x)


TALLIES = ("empty segment", "segment within cache", "segment longer than cache", "in-band cached", "in-band uncached",
           "band over two buckets", "third limb", "cache reused", "cache reloaded")


def classes(v, levels, lo, hi, tol=TOL, max_iter=None, fit=None):
    """dict(tallies = {class: boundary/iterate pairs}, gs, sum_path ('serial' up to 8 levels, 'tree' above), idle_groups,
    geometry, fit, pairs)."""
    s = _Sorted(v)
    g = s.g
    fit = fit or _fit(s.x, levels, lo, hi, tol, max_iter)
    gs = gs_of(levels)
    cache = CR * gs
    t = collections.Counter({k: 0 for k in TALLIES})
    prev = None
    for a in fit["alphas"]:
        vlo, vhi, jlo, jhi = _bands(g, levels, lo, hi, a)
        seg0, seg1 = s.cnt_below(jlo), s.cnt_below(jhi + 1)
        seglen = seg1 - seg0
        t["empty segment"] += int(np.count_nonzero(seglen == 0))
        t["segment within cache"] += int(np.count_nonzero((seglen > 0) & (seglen <= cache)))
        t["segment longer than cache"] += int(np.count_nonzero(seglen > cache))
        t["band over two buckets"] += int(np.count_nonzero(jhi > jlo))
        if prev is not None:
            same = (jlo == prev[0]) & (jhi == prev[1])
            t["cache reused"] += int(np.count_nonzero(same))
            t["cache reloaded"] += int(np.count_nonzero(~same))
        prev = (jlo, jhi)
        i_lo, i_hi = np.searchsorted(s.xs, vlo, side="right"), np.searchsorted(s.xs, vhi, side="left")
        i_hi = np.maximum(i_hi, i_lo)
        for ki in np.nonzero(i_hi > i_lo)[0]:
            # the in-band values of bucket j sit somewhere in [cnt_below(j), cnt_below(j + 1)): pigeonholes
            cached = uncached = False
            js, ms = np.unique(s.bk[i_lo[ki]:i_hi[ki]], return_counts=True)
            for j, m in zip(js, ms):
                start, c = int(s.cnt_below(j) - seg0[ki]), int(s.cnt_below(j + 1) - s.cnt_below(j))
                in_cache = min(max(cache - start, 0), c)
                cached |= m > c - in_cache
                uncached |= m > in_cache
            t["in-band cached"] += int(cached)
            t["in-band uncached"] += int(uncached)
        if gs > 1:
            # the values of the segment that lie below the band; some lane sums at least the gs-th part of their units
            nb = np.maximum(i_lo - seg0, 0)
            units = (s.csum[seg0 + nb] - s.csum[seg0] - nb * g.origin(jlo)) / g.q
            t["third limb"] += int(np.count_nonzero(units / gs >= 2.0 ** 42))
    return {"tallies": dict(t), "gs": gs, "sum_path": "serial" if levels <= 8 else "tree",
            "idle_groups": TI // gs - (levels - 1), "geometry": g, "fit": fit,
            "pairs": len(fit["alphas"]) * (levels - 1)}


def reached(cls):
    """The names of REQUIRED that one case reaches."""
    g, t = cls["geometry"], cls["tallies"]
    got = {f"k_fps<{g.inst}>" if g.path == "S" else "path G", f"gs = {cls['gs']}", f"level sum {cls['sum_path']}"}
    if g.path == "S":
        got.add(f"extra = {g.extra}")
    if cls["idle_groups"] > 0 and cls["gs"] < 64:
        got.add("idle groups")
    got |= {k for k in TALLIES if t[k] > 0}
    return got


REQUIRED = (("k_fps<8>", "k_fps<16>", "k_fps<32>", "path G") + tuple(f"gs = {x}" for x in (64, 32, 16, 8, 4, 2, 1))
            + ("level sum serial", "level sum tree", "idle groups") + tuple(f"extra = {x}" for x in range(8)) + TALLIES)


Layout = collections.namedtuple("Layout", "header tickets isum cnt tail total")


def workspace_layout(n):
    """Byte ranges [start, end) of fpg_carve: the header with its three tickets, the two tables that are zero between
    calls, and the tail of rank and grouped.  Up to S_MAXN values the kernel asks for 256 bytes and touches none."""
    if n <= S_MAXN:
        return Layout((0, 256), (4, 16), (256, 256), (256, 256), (256, 256), 256)
    p = 256
    isum = (p, p + 8 * MAXB)
    p = isum[1] + 8 * (MAXB + 2) + 8 * 2 * MAXBLK + 4096                 # spre, partials, the segment tables
    cnt = (p, p + 4 * MAXB)
    p = cnt[1] + 4 * (MAXB + 2)                                            # off
    tail = (p, p + (n + 64) * 8)
    return Layout((0, 256), (4, 16), isum, cnt, tail, tail[1])


# ---------------------------------------------------------------------------------------------------------- the cases
Case = collections.namedtuple("Case", "name section spec levels lo hi reaches")


def relu(n, seed):
    """Post-ReLU data: half exact zeros, with -0.0, -1e-30 and denormals among them."""
    x = np.maximum(R.normal(n, seed, sigma=0.3), f32(0))
    z = np.nonzero(x == 0)[0]
    x[z[0:40]] = f32(-0.0)
    x[z[40:80]] = f32(-1e-30)
    x[z[80:120]] = f32(1e-42)
    x[z[120:160]] = f32(-1e-42)
    return x


def outlier(n, seed, r):
    """One value of r mean|v| in a normal tensor."""
    x = R.normal(n, seed)
    x[0] = f32(r * float(np.abs(x.astype(np.float64)).mean()))
    return x


def copies_below_first_boundary(n, seed, copies, levels=4):
    """`copies` of one value in the bucket of the top boundary of the FIRST iterate (alpha_0 = mean|v| needs no fixed
    point), just above that bucket's lower edge: all of them below the boundary, all in its segment."""
    base = R.normal(n, seed)
    kpos = -1.0 + (levels - 1.5) * 2.0 / (levels - 1)
    c = f32(0.03)
    for _ in range(8):
        x = np.concatenate([base, np.full(copies, c, f32)])
        g = Geometry(x)
        t = float(np.abs(x.astype(np.float64)).mean()) * kpos
        j = int(g.bucket(f32(t)))
        c = f32(j * g.w - g.R64 + 0.05 * g.w)
    return np.concatenate([base, np.full(copies, c, f32)])


@functools.lru_cache(maxsize=None)
def _adversarial(levels):
    return R.adversarial(levels)


@functools.lru_cache(maxsize=4)
def tensor(spec):
    kind = spec[0]
    if kind == "normal":
        return R.normal(spec[1], spec[2])
    if kind == "clustered":
        return R.clustered(spec[1], spec[2])
    if kind == "adversarial":
        x = _adversarial(spec[1])[spec[2]]
        return np.concatenate([x, R.normal(40000, 77 + spec[1], sigma=0.1)]) if spec[3] else x
    if kind == "outlier":
        return outlier(spec[1], spec[2], spec[3])
    if kind == "copies":
        return copies_below_first_boundary(spec[1], spec[2], spec[3])
    if kind == "relu":
        return relu(spec[1], spec[2])
    raise ValueError(kind)


A_SIZES = (1, 5, 1024, 1025, 8192, 8193, 16384, 16385, 32768, 32769, 40960, 65537, 262147)
B_LEVELS = (2, 3, 4, 6, 8, 9, 16, 17, 33, 65, 129, 130, 255, 256)
C_LEVELS = (2, 3, 4, 5, 16, 256)
C_NAMES = ("boundaries", "zeros_tiny", "duplicates", "outlier", "all_equal", "two_values")
LADDER = ((60, 0), (70, 1), (130, 2), (300, 3), (600, 4), (2300, 5), (5000, 6), (20000, 7))   # (r, the extra it is for)


def _path(n):
    return "path G" if n > S_MAXN else "k_fps<%d>" % (8 if n <= 8192 else 16 if n <= 16384 else 32)


def _cases():
    out = []
    for n in A_SIZES:
        for kind in ("normal", "clustered"):
            out.append(Case(f"{kind}-{n}", "a", (kind, n, 5 * n + 1), 4, -1.0, 1.0, (_path(n),)))
    out.append(Case(f"clustered-{MAXN}", "a", ("clustered", MAXN, 23), 4, -1.0, 1.0, ("path G",)))
    for L in B_LEVELS:
        for n in (12000, 36000):
            want = [_path(n), f"gs = {gs_of(L)}", "level sum serial" if L <= 8 else "level sum tree"]
            if L == 4:
                want += ["segment within cache", "cache reused", "cache reloaded"]
            if L == 16:
                want.append("empty segment")
            if L == 6:
                want.append("idle groups")
            if L >= 33:
                want.append("band over two buckets")
            if L >= 65:
                want.append("segment longer than cache")
            out.append(Case(f"L{L}-{n}", "b", ("normal", n, 3 * n + L), L, -1.0, 1.0, tuple(want)))
    for L in C_LEVELS:
        for name in C_NAMES:
            for big in (False, True):
                # (the boundary points of 256 levels and ~230 iterates are 400 000 values on their own)
                want = ["path G" if big or (name == "boundaries" and L == 256) else "k_fps<32>"]
                if name == "boundaries" and L % 2 == 0:                      # the points ON the boundary at zero
                    want.append("in-band cached" if L <= 16 else "in-band uncached")
                if name == "zeros_tiny" and L % 2 == 0:
                    want.append("in-band uncached")                          # 1300 values in the band around zero
                if name == "outlier" and not big:
                    want += ["extra = 7"] + (["third limb"] if L in (3, 4, 5, 16) else [])
                if name == "duplicates" and L == 16 and not big:
                    want += ["extra = 0", "third limb"]
                out.append(Case(f"{name}-L{L}-{'appended' if big else 'alone'}", "c", ("adversarial", L, name, big), L, -1.0, 1.0,
                                tuple(want)))
    for r, extra in LADDER:
        out.append(Case(f"outlier-x{r}", "c", ("outlier", 12000, 900 + r, r), 4, -1.0, 1.0, (f"extra = {extra}", "k_fps<16>")))
    out.append(Case("copies-G", "c", ("copies", 40000, 41, 8192), 4, -1.0, 1.0, ("path G", "gs = 64", "third limb")))
    for L, n in ((4, 12000), (16, 12000), (256, 12000), (16, 36000)):
        out.append(Case(f"relu-L{L}-{n}", "d", ("relu", n, 7 * n + L), L, 0.0, 1.0, (_path(n),)))
    for L, n in ((4, 12000), (16, 36000)):
        out.append(Case(f"signed-on-unsigned-L{L}-{n}", "d", ("normal", n, 9 * n + L), L, 0.0, 1.0, (_path(n),)))
    return tuple(out)


CASES = _cases()


def section(s):
    return [c for c in CASES if c.section == s]
