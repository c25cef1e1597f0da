"""The bracketed activation-scale fit (csrc/fixed_point_bracket.hip) pass by pass against exact integers.

The kernel rests on one invariant - decided tallies + undecided list = the whole tensor, at every pass - and its planner
only decides what is worth doing, so a pass that drops or double-counts a few values still converges in the same number
of steps to an alpha inside the parity bar.  Here the C entry points are stepped ONE iteration at a time on a workspace
the test owns, and after every iteration the two sums, the state, the decided tallies and the compacted list are held to
tests/fp_bracket_ref.py: integers exactly, the fp64 sums to a bound derived from the number of roundings.  Every case
asserts from the header counters that it reached the pass class it is there for.

Measured on an MI355X, finished fits against oracle.effq_oracle.fit_scale (iteration counts equal in every case; bar
1e-11), the relative difference of alpha and the iterations it took:
  relu 20011 L=2 0.0 (13) | L=4 2.6e-16 (29) | L=16 1.8e-16 (90, 6 escapes) | relu 8193 L=256 2.9e-16 (368, 52 escapes) |
  signed 16389 L=16 2.9e-16 (61, 3 escapes) | bimodal 12289 L=8 2.6e-16 (33, widen 1) | five-valued 12289 L=4 0.0 (6, widen 1) |
  adversarial L=4 1.3e-16 (24) | n=3 0.0 (3) | n=37 2.2e-16 (3) | n=8192 1.3e-16 (28) | n=8193 2.5e-16 (22) | unaligned view 0.0 (30)
Three unequal shards: 27 iterations at 4 levels, 12 of them all-reduced; 173 at 16 levels, 158 all-reduced, three
distinct brackets intersected at the accepted exchange; both end at the unsharded fit's count and within 1e-13 of its alpha."""
import math

import numpy as np
import pytest
import torch

from oracle import effq_oracle as O
from tests import fp_bracket_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5                                    # ADMM_TOL
X, A, B, Z = 0, 1, 2, 3                       # sources: the tensor, the two working lists, the base list
GARBAGE = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_ops("cuda:0")


class Header:
    """The words of FbrHdr (a test-local reader: the whole header, where ops.fp_bracket_diagnostics picks some)."""
    F = {"blo": 0, "bhi": 1, "nlo": 2, "nhi": 3, "alpha_pp": 4, "inv_q": 5, "q": 6, "guard_lo": 23, "guard_hi": 24}
    I = {"src": 7, "dst": 8, "narrow": 9, "G": 10, "per": 11, "escapes": 12, "narrowings": 13, "visited": 14,
         "list_total": 15, "mono": 18, "planned": 19, "widen": 20, "base": 21, "z_total": 22}

    def __init__(self, raw):
        f, i = raw.view(torch.float64), raw.view(torch.int64)
        for k, j in self.F.items():
            setattr(self, k, float(f[j]))
        for k, j in self.I.items():
            setattr(self, k, int(i[j]))
        self.ext = tuple(int(x) for x in i[25:29])


class State:
    def __init__(self, st):
        host = st.cpu()
        self.alpha, self.alpha_prev, s0, s1 = (float(x) for x in host[:4])
        self.sums = (s0, s1)
        self.iters, self.done = (int(x) for x in host[4:5].view(torch.int32))

    def key(self):
        return (self.alpha, self.alpha_prev, self.sums, self.iters, self.done)


class Fit:
    """One fit on a workspace and a state of its own, driven through the C entry points."""

    def __init__(self, ops, v, L, lo, hi, abs_sums, offset=0, st=None, init=True):
        from efficientq_amd.hip_ops import _ptr
        from efficientq_amd._lib import check
        self.ops, self.lib, self.stream, self._ptr, self._check = ops, ops.lib, ops.stream, _ptr, check
        self.L, self.lo, self.hi, self.n = L, float(lo), float(hi), int(v.size)
        store = torch.zeros(self.n + offset, dtype=torch.float32, device="cuda:0")
        self.x = store[offset:]                                  # offset 1: a view 4 bytes past a 16-byte boundary
        self.x.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)))
        assert self.x.data_ptr() % 16 == 4 * offset
        self.max_iter = 100 * L
        self.st = ops.new_fp_state() if st is None else st
        self.ws = torch.zeros(self.lib.effq_fp_bracket_ws_bytes(self.n), dtype=torch.uint8, device="cuda:0")
        if init:
            s0 = torch.tensor([float(abs_sums[0]), float(abs_sums[1])], dtype=torch.float64, device="cuda:0")
            check(self.lib.effq_fp_bracket_init(_ptr(self.st), _ptr(s0), self.n, L, int(lo == 0.0), _ptr(self.ws),
                                                self.ws.numel(), self.stream), "init")

    def header(self):
        return Header(self.ws[:256].cpu())

    def state(self):
        return State(self.st)

    def run(self, iters=1):
        self._check(self.lib.effq_fp_bracket_run(self._ptr(self.x), self.n, self.L, self.lo, self.hi, TOL, self.max_iter,
                                                 iters, self._ptr(self.st), self._ptr(self.ws), self.stream), "run")

    def stats(self):
        self._check(self.lib.effq_fp_bracket_stats(self._ptr(self.x), self.n, self.L, self.lo, self.hi, self._ptr(self.st),
                                                   self._ptr(self.ws), self.stream), "stats")

    def set_sums(self, sums):
        self.st[2:4] = torch.tensor(sums, dtype=torch.float64)

    def update(self):
        self._check(self.lib.effq_fp_bracket_update(self.n, self.L, self.lo, self.hi, TOL, self.max_iter,
                                                    self._ptr(self.st), self._ptr(self.ws), self.stream), "update")

    def export(self, cap):
        """(out words, list buffer) as numpy, both garbage-filled before the call."""
        out = torch.full((self.lib.effq_fp_bracket_export_words(),), GARBAGE, dtype=torch.int64, device="cuda:0")
        lst = torch.full((cap,), 7.0, dtype=torch.float32, device="cuda:0")
        self._check(self.lib.effq_fp_bracket_export(self._ptr(self.ws), self.n, self._ptr(out), self._ptr(lst), cap,
                                                    self.stream), "export")
        return out.cpu().numpy(), lst.cpu().numpy()

    def imported(self, pack, world, slot, gathered):
        """The fit over the gathered lists that this rank finishes on its own (same state)."""
        f = Fit(self.ops, gathered, self.L, self.lo, self.hi, None, st=self.st, init=False)
        p = torch.tensor(pack, dtype=torch.int64, device="cuda:0")
        self._check(self.lib.effq_fp_bracket_import(self._ptr(self.ws), self.n, self._ptr(p), world, slot, self._ptr(self.st),
                                                    self._ptr(f.ws), f.ws.numel(), self.stream), "import")
        return f

    def rebase(self):
        self._check(self.lib.effq_fp_bracket_rebase(self._ptr(self.st), self._ptr(self.ws), self.n, self.stream), "rebase")


class Ref:
    """The yardstick's view of one tensor: values, integer units, and the undecided mask per bracket."""

    def __init__(self, v, L, lo, hi, sum_abs):
        self.n, self.L, self.lo, self.hi = int(v.size), L, float(lo), float(hi)
        self.d = (self.hi - self.lo) / (L - 1)
        self.e = R.unit_exponent(L, sum_abs)
        self.q = math.ldexp(1.0, -self.e)
        v = np.ascontiguousarray(v, dtype=np.float32)
        if lo == 0.0:
            # an exact zero of either sign has level 0 and unit 0 at every scale a > 0: it adds nothing to any tally and is
            # never undecided (pinned in test_fp_bracket_ref_cpu.py), so the per-pass work leaves the zeros out
            v = v[v != 0.0]
        self.v32 = v
        self.x = v.astype(np.float64)
        self.u = R.units(v, self.e)
        self._und = {}

    def tallies(self, a, mask=None):
        return R.tallies(self.x, self.u, a, self.lo, self.hi, self.d, mask)

    def undecided(self, blo, bhi):
        key = (blo, bhi)
        if key not in self._und:
            self._und = {key: R.undecided(self.x, blo, bhi, self.lo, self.hi, self.d)}       # (keeps the last one only)
        return self._und[key]


def abs_sum(*vs):
    """sum |v| over all the shards, correctly rounded: alpha_0 = abs_sum / n is then known exactly."""
    return math.fsum(t for v in vs for t in np.abs(np.asarray(v, dtype=np.float64)).tolist())


def check_sums(sums, ref, a, n, what):
    """state.sums of a pass that classified at scale a, against the exact sums over the tensor of `ref`."""
    _, exact, absolute = R.sums_from_tallies(ref.tallies(a), n, ref.lo, ref.d, ref.q)
    assert R.within(sums[0], exact[0], absolute[0], 4), (what, "sum b v", sums[0], float(exact[0]))
    assert R.within(sums[1], exact[1], absolute[1], 8), (what, "sum b b", sums[1], float(exact[1]))


def check_export(fit, ref, what, cap=None):
    """The export of a fit against the tensor of `ref`.  Returns out[4]."""
    h = fit.header()
    if cap is None:
        cap = (h.list_total if h.src != X else 4096) + 13          # no multiple of G: the zero-fill is partitioned raggedly
    out, lst = fit.export(cap)
    blo, bhi = (float(t) for t in out[5:7].view(np.float64))
    assert (blo, bhi) == (h.blo, h.bhi), what
    length = int(out[4])
    if h.src == X:
        # the next pass reads the whole tensor: nothing is decided, whatever an earlier bracket had settled
        assert tuple(int(t) for t in out[:4]) == (0, 0, 0, 0), (what, "decided tallies", out[:4].tolist(), vars(h))
        assert length == -1 and h.list_total == 0, (what, length, h.list_total)
        assert not lst.any(), (what, "no list handed out: zero-filled")
        return length
    und = ref.undecided(blo, bhi)
    want = ref.tallies(blo, ~und)                                  # (decided: the same level at every scale inside)
    assert tuple(int(t) for t in out[:4]) == want, (what, "decided tallies", out[:4].tolist(), want, vars(h))
    count = int(und.sum())
    assert h.list_total == count, (what, h.list_total, count)
    if h.planned != 0:
        assert length == -2, (what, length)
    else:
        assert length == count, (what, length, count)
    if 0 <= length <= cap:
        got, want_list = np.sort(lst[:length]), np.sort(ref.v32[und])
        assert np.array_equal(got, want_list), (what, "list content")
        assert np.array_equal(np.signbit(got), np.signbit(want_list))
        assert not lst[length:].any(), (what, "behind the list")
    else:
        assert not lst.any(), (what, "no list handed out: zero-filled")
    return length


def step(fit, ref, k, what, export=True):
    """Iteration k of `fit` with every per-pass check against `ref`.  Returns (state, out[4] or None)."""
    a = fit.state().alpha
    fit.run(1)
    s, h = fit.state(), fit.header()
    assert h.inv_q == math.ldexp(1.0, ref.e) and h.q == ref.q, (what, h.inv_q, ref.e)
    check_sums(s.sums, ref, a, fit.n, what)
    assert s.alpha == s.sums[0] / s.sums[1] and s.alpha_prev == a, (what, vars(s))
    assert s.iters == k, (what, s.iters)
    done = R.stop(k, fit.max_iter, s.alpha, a, TOL)
    if done == 0 and not (h.guard_lo <= s.alpha <= h.guard_hi):
        done = 4
    assert s.done == done, (what, s.done, done)
    return s, (check_export(fit, ref, what) if export else None)


def drive(ops, v, L, lo, hi, what, offset=0, max_steps=None, oracle=True):
    """A whole fit, stepped and checked; returns (header at the end, export lengths seen, header history)."""
    S = abs_sum(v)
    fit, ref = Fit(ops, v, L, lo, hi, (S, v.size), offset=offset), Ref(v, L, lo, hi, S)
    s0, h0 = fit.state(), fit.header()
    assert s0.alpha == S / v.size and (s0.iters, s0.done) == (0, 0)
    assert (h0.G, h0.per) == R.shape(v.size), (what, h0.G, h0.per)
    check_export(fit, ref, f"{what} before the first pass")
    lengths, hist = [], []
    for k in range(1, (max_steps or fit.max_iter) + 1):
        s, length = step(fit, ref, k, f"{what} iteration {k}")
        lengths.append(length)
        hist.append(fit.header())
        if s.done:
            break
    if max_steps is None:
        assert s.done == 1, (what, s.done)
    if oracle and max_steps is None:
        want = O.fit_scale(torch.from_numpy(np.ascontiguousarray(v)), L, lo, hi)
        rel = abs(s.alpha - want.alpha) / abs(want.alpha)
        print(f"\n{what}: {s.iters} iterations, alpha rel diff to the oracle {rel:.1e}; escapes {hist[-1].escapes} "
              f"narrowings {hist[-1].narrowings} widen {hist[-1].widen} visited {hist[-1].visited}")
        assert s.iters == want.iters, (what, s.iters, want.iters)
        assert rel <= 1e-11, (what, s.alpha, want.alpha)
    return hist[-1], lengths, hist


# ---- pass classes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 2])
def test_base_list_build_narrowings_and_plain_list_passes(ops, L):
    h, lengths, hist = drive(ops, R.relu(20011), L, 0.0, 1.0, f"relu 20011 L={L}")
    assert h.base == Z and h.narrowings >= 5 and h.escapes == 0, vars(h)
    srcs = [x.src for x in hist]
    assert A in srcs and B in srcs                                                  # narrowed both ways
    assert any(a.src == b.src and a.narrowings == b.narrowings for a, b in zip(hist, hist[1:]))     # plain list passes
    assert min(t for t in lengths if t >= 0) < h.z_total // 4


@pytest.mark.parametrize("n,L", [(20011, 16), (8193, 256)])
def test_horizon_brackets_planned_escapes_and_rebuilds_from_the_base_list(ops, n, L):
    h, lengths, hist = drive(ops, R.relu(n), L, 0.0, 1.0, f"relu {n} L={L}")
    assert h.base == Z and h.escapes >= 1 and h.widen == 0, vars(h)
    assert -2 in lengths
    # right after an escape the source is the base list again, with the bracket of the base
    esc = [b for a, b in zip(hist, hist[1:]) if b.escapes == a.escapes + 1]
    assert esc and all(x.src == Z and x.list_total == x.z_total and (x.blo, x.bhi) == (1e-300, 1e300) for x in esc)


def test_base_is_the_tensor_and_rebuilds_read_it_again(ops):
    h, lengths, hist = drive(ops, R.signed(16389), 16, -1.0, 1.0, "signed 16389 L=16")
    assert h.base == X and h.escapes >= 1 and h.z_total == 0, vars(h)
    assert lengths[0] == -1 and any(t >= 0 for t in lengths)


@pytest.mark.parametrize("name,L", [("bimodal", 8), ("five", 4)])
def test_escape_from_a_bracket_that_was_to_hold_the_limit(ops, name, L):
    v = R.bimodal(12289) if name == "bimodal" else R.five_valued(12289)
    h, lengths, hist = drive(ops, v, L, 0.0, 1.0, f"{name} 12289 L={L}")
    assert h.widen >= 1 and h.escapes >= 1, vars(h)


# ---- slice shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,offset", [(3, 0), (37, 0), (8192, 0), (8193, 0), (20011, 1)])
def test_slice_shapes(ops, n, offset):
    """Fewer values than one 16-byte load: the tail loop alone; one workgroup with one partly filled vector step and a tail
    of one value; exactly one full slice; two slices, the second ragged; a view 4 bytes past a 16-byte boundary (scalar
    first pass over the tensor, vector passes over the lists, which are aligned)."""
    h, lengths, hist = drive(ops, R.relu(n, seed=n), 4, 0.0, 1.0, f"relu {n} offset {offset}", offset=offset)
    assert (h.G, h.per) == {3: (1, 4), 37: (1, 40), 8192: (1, 8192), 8193: (2, 4100), 20011: (3, 6672)}[n]
    assert h.base == Z and h.narrowings >= 2


def test_slice_grid_at_its_cap(ops):
    """8 Mi + 5 values: 1024 workgroups of 8196 values, a short last slice; the first four iterations only."""
    n = 8 * 2 ** 20 + 5
    h, lengths, hist = drive(ops, R.relu(n, seed=8), 4, 0.0, 1.0, "relu 8Mi+5", max_steps=4, oracle=False)
    assert (h.G, h.per) == (1024, 8196) and h.base == Z and h.narrowings >= 2, vars(h)
    assert lengths[0] == h.z_total and h.src in (A, B) and 0 < h.list_total < h.z_total


def test_adversarial_values(ops):
    """Values on the level boundaries of the first scales the fit classifies at and one ulp either side (the fp32 screen
    cannot settle them: the fp64 fallback decides), tiny non-zeros (on the base list), negative zeros and negatives under
    lo = 0 (never listed)."""
    v = R.adversarial(4)
    h, lengths, hist = drive(ops, v, 4, 0.0, 1.0, "adversarial L=4")
    assert h.base == Z and h.z_total == int((v > 0).sum()), vars(h)
    # the case reached what it is there for: at the scales the KERNEL classified at in its first passes (alpha_pp of the
    # header two iterations on), the tensor's triples lie one ulp either side of every boundary
    bits = v.view(np.uint32)
    for j in range(R.ADVERSARIAL_SCALES):
        a = hist[j + 1].alpha_pp
        tr = R.boundary_triples(a, 4)
        lv = R.level(tr.astype(np.float64), a, 0.0, 1.0, 1.0 / 3.0)
        assert np.isin(tr.view(np.uint32), bits).all() and lv[0].tolist() == [0, 1, 2] and lv[2].tolist() == [1, 2, 3], j


# ---- the exchange between data-parallel ranks, emulated on one device ----------------------------------------------
class Ranks:
    """Shards of one tensor, one Fit each, iterating in lock step on the all-reduced sums."""

    def __init__(self, ops, shards, L):
        self.shards, self.L = shards, L
        self.union = np.concatenate(shards)
        self.S = abs_sum(*shards)
        tot = (self.S, self.union.size)
        self.fits = [Fit(ops, p, L, 0.0, 1.0, tot) for p in shards]
        self.refs = [Ref(p, L, 0.0, 1.0, self.S) for p in shards]
        self.uref = Ref(self.union, L, 0.0, 1.0, self.S)
        self.k = 0
        whole = Fit(ops, self.union, L, 0.0, 1.0, tot)          # the unsharded fit
        for _ in range(100 * L):
            whole.run(8)
            self.want = whole.state()
            if self.want.done:
                break
        assert self.want.done == 1

    def reduced_iteration(self):
        """One all-reduced iteration with the per-pass checks on every rank's own sums.  Returns the state."""
        self.k += 1
        a = self.fits[0].state().alpha
        parts = []
        for i, (f, r) in enumerate(zip(self.fits, self.refs)):
            f.stats()
            parts.append(f.state().sums)
            check_sums(parts[-1], r, a, f.n, f"rank {i} iteration {self.k}")
        both = (sum(p[0] for p in parts), sum(p[1] for p in parts))
        for f in self.fits:
            f.set_sums(both)
            f.update()
        states = [f.state() for f in self.fits]
        assert all(s.key() == states[0].key() for s in states)                       # ranks in lock step
        s = states[0]
        assert s.alpha == both[0] / both[1] and s.iters == self.k and s.done == R.stop(self.k, 100 * self.L, s.alpha, a, TOL)
        return s

    def exchange(self, slot, checked=True):
        """Export (with the export checks), pack, import; every rank runs the imported fit, rank 0 with the per-pass checks
        against the UNION tensor.  Returns the common state: done = 1, or 4 if the exchange was refused or left."""
        packs, lists = [], []
        for i, (f, r) in enumerate(zip(self.fits, self.refs)):
            if checked:
                check_export(f, r, f"rank {i} export after iteration {self.k}", cap=slot)
            out, lst = f.export(slot)
            packs.append(out)
            lists.append(lst)
        world = len(self.fits)
        pack = [sum(int(p[j]) for p in packs) for j in range(4)] + [int(p[j]) for p in packs for j in (4, 5, 6)]
        gathered = np.concatenate(lists)                         # what the all-gather leaves on every rank
        usable = all(0 <= int(p[4]) <= slot for p in packs)
        res = []
        for i, f in enumerate(self.fits):
            before = f.state()
            g = f.imported(pack, world, slot, gathered)
            self.accepted = g.state().done == 0
            if not usable:
                assert not self.accepted
            k = self.k
            for _ in range(100 * self.L):
                if i == 0 and g.state().done == 0:
                    k += 1
                    s, _ = step(g, self.uref, k, f"imported fit iteration {k}", export=False)
                else:
                    g.run(8)
                    s = g.state()
                if s.done:
                    break
            if not usable:
                assert s.key() == (before.alpha, before.alpha_prev, before.sums, before.iters, 4)      # run changed nothing
            res.append(s)
        assert all(s.key() == res[0].key() for s in res), [s.key() for s in res]   # bit-identical ranks
        if res[0].done == 4:
            # the state goes on from where the imported fit stopped; the ranks' own lists are rebuilt from their bases
            for f in self.fits:
                f.rebase()
            self.k = res[0].iters
            assert all(f.state().done == 0 for f in self.fits)
        return res[0]

    def finish_reduced(self):
        s = self.fits[0].state()
        while not s.done:
            s = self.reduced_iteration()
        return s

    def assert_ends_where_the_unsharded_fit_ends(self, s):
        assert s.done == 1 and s.iters == self.want.iters, (s.key(), self.want.key())
        assert abs(s.alpha - self.want.alpha) <= 1e-13 * self.want.alpha, (s.alpha, self.want.alpha)


@pytest.mark.parametrize("L", [4, 16])
def test_exchange_between_three_unequal_shards(ops, L):
    """Shards of 9001, 20011 and 300 values: 2, 3 and 1 workgroups, and at 16 levels brackets that differ between the ranks
    (each plans its horizons on its own shard's density): the import intersects them."""
    v = R.relu(9001 + 20011 + 300, seed=31)
    ranks = Ranks(ops, [v[:9001], v[9001:29012], v[29012:]], L)
    assert [f.header().G for f in ranks.fits] == [2, 3, 1]
    slot, finished, distinct = 20012, 0, 0
    s = ranks.fits[0].state()
    while not s.done:
        for _ in range(4):
            s = ranks.reduced_iteration()
            if s.done:
                break
        if s.done:
            break
        brackets = {(f.header().blo, f.header().bhi) for f in ranks.fits}
        s = ranks.exchange(slot)
        if ranks.accepted:
            distinct = max(distinct, len(brackets))
        if s.done == 1:
            finished += 1
        else:
            s = ranks.fits[0].state()
    print(f"\nL={L}: {s.iters} iterations, {ranks.k} of them all-reduced, finished on the gathered lists: {finished}, "
          f"distinct brackets at an accepted exchange: {distinct}")
    if L == 4:
        assert finished == 1 and ranks.k < s.iters               # the rest of the iterations needed no collective
    ranks.assert_ends_where_the_unsharded_fit_ends(s)


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("kind,L", [("relu", 16), ("bimodal", 8)])
def test_export_right_after_an_escape(ops, kind, L, world):
    """All-reduced iterations until a rank's iterate has just left its bracket: the next pass starts from the base list,
    so the export must not offer the tallies of the bracket it left together with that whole list.  At 16 levels the
    escape is a planned one and the plan that follows is as a rule a horizon again (the export says -2); the bimodal
    tensor at 8 levels leaves a bracket that was to hold the limit, the plan that follows is no horizon, and the export
    hands out the whole base list: the import that follows counts on its tallies."""
    v = R.relu(20011 + 9001, seed=32) if kind == "relu" else R.bimodal(12289)
    ranks = Ranks(ops, ([v[:20011], v[20011:]] if kind == "relu" else [v[0::2], v[1::2]]) if world == 2 else [v], L)
    before = [0] * world
    for _ in range(100 * L):
        s = ranks.reduced_iteration()
        now = [f.header().escapes for f in ranks.fits]
        if s.done or now != before:
            break
        before = now
    assert not s.done and now != before, "no escape before the end: the case tests nothing"
    lengths = []
    for i, (f, r) in enumerate(zip(ranks.fits, ranks.refs)):
        lengths.append(check_export(f, r, f"rank {i} right after the escape"))
        h = f.header()
        if now[i] != before[i]:
            assert h.src == Z and h.list_total == h.z_total and lengths[-1] == (-2 if h.planned else h.z_total)
    if kind == "bimodal":
        assert min(lengths) > 0                                  # the case is there for an import after the escape
    s = ranks.exchange(29012)
    assert ranks.accepted == (min(lengths) >= 0)
    if s.done != 1:
        s = ranks.finish_reduced()
    ranks.assert_ends_where_the_unsharded_fit_ends(s)


@pytest.mark.parametrize("short", [0, 1])
def test_slot_of_exactly_the_list_and_one_float_less(ops, short):
    v = R.relu(20011 + 9001, seed=33)
    ranks = Ranks(ops, [v[:20011], v[20011:]], 4)
    for _ in range(40):                                          # until every rank has a list it would hand out
        s = ranks.reduced_iteration()
        hs = [f.header() for f in ranks.fits]
        if s.done or all(h.src in (A, B) and h.planned == 0 for h in hs):
            break
    assert not s.done and all(h.src in (A, B) and h.planned == 0 and h.list_total > 1 for h in hs), [vars(h) for h in hs]
    longest = max(h.list_total for h in hs)
    if short == 0:
        # the zero-fill behind the list, split over G = 3 workgroups at every remainder (and with nothing to fill)
        for extra in (0, 1, 2, 3, 4, 1001):
            check_export(ranks.fits[0], ranks.refs[0], f"cap = list + {extra}", cap=hs[0].list_total + extra)
        s = ranks.exchange(longest)
        assert ranks.accepted
        if s.done != 1:
            s = ranks.finish_reduced()
    else:
        k = ranks.k
        s = ranks.exchange(longest - 1)                          # the longest list does not fit: refused on the device
        assert s.done == 4 and s.iters == k and not ranks.accepted
        s = ranks.finish_reduced()
    ranks.assert_ends_where_the_unsharded_fit_ends(s)
