"""effq_fixed_point_bucket_rec (csrc/fixed_point_bucket.hip, the recorder and the stop rule of csrc/fp_level.h) class by class
against fp64 (-m gpu).  Which path, which k_fps instantiation, which lane grouping, which kind of boundary segment and
which integer unit a case reaches is derived in tests/fp_bucket_ref.py and vouched for without a GPU by
tests/test_fp_bucket_ref_cpu.py; every case of sections a to d here is a row of fp_bucket_ref.CASES.

  a. build paths: k_fps<8 / 16 / 32> and the four launches, from one value to the admitted 2^23;
  b. iteration geometry: every lane grouping (64 .. 1 lanes per boundary), both level-sum paths, idle groups;
  c. boundary segments and integer sums: values on boundaries, zeros, denormals, duplicates, the outlier ladder of the
     finer units, the third limb of the group sum;
  d. the unsigned grid on ReLU and on signed data;
  e. the three operand modes, each operand one float off 16-byte alignment;
  f. the stop rule: the cap, tensors without a scale;
  g. one workspace across sizes, scales and paths;
  h. the refusals.

Every call runs inside sentinel bands (v_out NaN-prefilled between 64-float guards; state, prediction and a workspace of
exactly effq_fp_bucket_ws_bytes(n) bytes between 256 guard bytes), once on a zero workspace and once on one that is 0xFF
wherever the contract does not ask for zeros: equal bits, guards untouched, tickets and the two counter tables back to zero.
A call is held to fp_traj_ref.iterates: done and the iteration count equal, alpha, alpha_prev and sum b v within 1e-11, sum
b^2 within 4 L 2^-53 of the sum over the direct level counts (at most L non-negative terms, each with at most three fp64
roundings; one miscounted value moves it by orders more), the recorded prediction equal to fp_traj_ref.record."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

from tests import fp_bucket_ref as F
from tests import fp_traj_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                       # floats on either side of v_out (keeps it 256-byte aligned)
SENTINEL = -7.25e33
BYTE = 0xA5                      # guard bytes around the workspace, the state and the prediction
TOL = 1e-5
PRED_BYTES = 16 + 8 * 63
PRED_CMP = 16 + 8 * 55           # everything before the time stamps
ERR_ARG, ERR_WORKSPACE = 1, 3
WORST = {}                       # section -> worst relative deviation of alpha seen (printed when the module ends)


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert get_ops(DEV).lib.effq_fp_traj_pred_bytes() == PRED_BYTES
    t0 = time.time()
    yield get_ops(DEV)
    print(f"\ntest_fp_bucket_classes_gpu: {time.time() - t0:.1f} s; worst |alpha - ref| / ref per section: "
          + ", ".join(f"{k}: {v:.2e}" for k, v in sorted(WORST.items())))


def dev(x, offset=0):
    """The vector on the device, `offset` floats off the 256-byte alignment of an allocation."""
    if x is None:
        return None
    buf = torch.empty(x.size + offset, dtype=torch.float32, device=DEV)
    buf[offset:].copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return buf[offset:]


def _note(section, got, want):
    rel = abs(got - want) / abs(want)
    WORST[section] = max(WORST.get(section, 0.0), rel)
    return rel


def _guarded(numel, offset=0):
    buf = torch.full((numel + 2 * GUARD + offset,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[GUARD + offset:GUARD + offset + numel]
    view.fill_(float("nan"))
    return buf, view


def _guards_untouched(buf, view_numel, offset=0):
    head, tail = buf[:GUARD + offset], buf[GUARD + offset + view_numel:]
    return bool((head == SENTINEL).all().item()) and bool((tail == SENTINEL).all().item())


def _bytes_between(nbytes):
    buf = torch.full((nbytes + 512,), BYTE, dtype=torch.uint8, device=DEV)
    return buf, buf[256:256 + nbytes]


def _bytes_untouched(buf):
    return bool((buf[:256] == BYTE).all().item()) and bool((buf[-256:] == BYTE).all().item())


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _workspace(lib, n, fill):
    """Exactly effq_fp_bucket_ws_bytes(n) bytes between guards: zero where the contract says so, `fill` elsewhere."""
    lay = F.workspace_layout(n)
    assert lib.effq_fp_bucket_ws_bytes(n) == lay.total
    buf, ws = _bytes_between(lay.total)
    ws.fill_(fill)
    for lo, hi in (lay.header, lay.isum, lay.cnt):
        ws[lo:hi] = 0
    return buf, ws


class Run:
    pass


def _once(ops, a, b, L, lo=-1.0, hi=1.0, max_iter=None, mode="av", v_off=0, fill=0x00, pred=None, ws_keep=None):
    """One guarded call.  mode: 'a' (no v_out), 'av', 'abv'.  -> Run"""
    lib, n = ops.lib, a.numel()
    r = Run()
    r.ws_buf, r.ws = _workspace(lib, n, fill) if ws_keep is None else ws_keep
    a0, b0 = a.clone(), None if b is None else b.clone()
    vbuf, v = _guarded(n, v_off) if mode != "a" else (None, None)
    sbuf, sview = _bytes_between(40)
    sview.fill_(0xFF)
    pbuf, pview = _bytes_between(PRED_BYTES)
    pview.copy_(ops.new_fp_pred() if pred is None else pred)
    rc = lib.effq_fixed_point_bucket_rec(_ptr(a), _ptr(b), _ptr(v), n, L, lo, hi, TOL, 100 * L if max_iter is None else max_iter,
                                         _ptr(sview), _ptr(r.ws), r.ws.numel(), _ptr(pview), ops.stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _bytes_untouched(r.ws_buf), "wrote outside the workspace"
    assert _bytes_untouched(sbuf), "wrote outside the state"
    assert _bytes_untouched(pbuf), "wrote outside the prediction"
    assert v is None or _guards_untouched(vbuf, n, v_off), "wrote outside v_out"
    assert torch.equal(a.view(torch.int32), a0.view(torch.int32)), "a changed"
    assert b is None or torch.equal(b.view(torch.int32), b0.view(torch.int32)), "b changed"
    lay = F.workspace_layout(n)
    assert r.ws[lay.tickets[0]:lay.tickets[1]].view(torch.int32).tolist() == [0, 0, 0], "tickets not back to zero"
    assert not bool(r.ws[lay.isum[0]:lay.isum[1]].any()), "isum not back to zero"
    assert not bool(r.ws[lay.cnt[0]:lay.cnt[1]].any()), "cnt not back to zero"
    st = sview.clone().view(torch.float64)
    r.state_bits = st.view(torch.int64).cpu().tolist()
    r.alpha, r.alpha_prev, r.sbv, r.sbb = (float(x) for x in st[:4].cpu())
    _, r.it, r.done = ops.read_fp_state(st)
    r.pred_dev = pview.clone()
    r.pred = ops.read_fp_pred(r.pred_dev)
    r.v = v
    return r


def _same(r1, r2):
    assert r1.state_bits == r2.state_bits, "the state differs in bits"
    assert torch.equal(r1.pred_dev[:PRED_CMP], r2.pred_dev[:PRED_CMP]), "the prediction differs"
    assert (r1.v is None) == (r2.v is None)
    if r1.v is not None:
        assert torch.equal(r1.v.view(torch.int32), r2.v.view(torch.int32)), "v_out differs"


def _call(ops, a, b, L, **kw):
    """On a zero workspace, then on one that is 0xFF behind the ranges the contract zeroes: equal bits.  -> Run"""
    r1 = _once(ops, a, b, L, fill=0x00, **kw)
    r2 = _once(ops, a, b, L, fill=0xFF, **kw)
    _same(r1, r2)
    return r1


def _same_bits_or_both_nan(x, y):
    return (math.isnan(x) and math.isnan(y)) or np.float64(x).view(np.int64) == np.float64(y).view(np.int64)


def _check(section, run, v_host, L, lo, hi, max_iter=None, count_margin=True):
    """The bars of the module's docstring on one Run.  -> fit"""
    max_iter = 100 * L if max_iter is None else max_iter
    fit = R.iterates(v_host, L, lo, hi, TOL, max_iter)
    if count_margin:
        assert fit["stop_margin"] > 1e-9, "the case's stop decision is a coin toss: choose another tensor"
    assert (run.done, run.it) == (fit["done"], fit["it"]), (run.done, run.it, fit["done"], fit["it"])
    before = R.cold_pred()
    want = R.record(before, fit["alphas"], fit["alpha"], fit["sum_abs"], L)
    got = run.pred
    assert (got["K"], got["e"], got["e_valid"], got["calls"]) == (want["K"], want["e"], want["e_valid"], 1), (got, want)
    if fit["it"] == 0:                                        # no scale: nothing was classified
        assert _same_bits_or_both_nan(run.alpha, fit["alpha"]), (run.alpha, fit["alpha"])
        return fit
    rel = _note(section, run.alpha, fit["alpha"])
    rel_prev = abs(run.alpha_prev - fit["alphas"][-1]) / fit["alphas"][-1]
    want_bv = F.sum_bv(v_host, L, lo, hi, fit["alphas"][-1])
    want_bb = F.sum_bb(F.level_counts(v_host, L, lo, hi, fit["alphas"][-1]), L, lo, hi)
    rel_bv, rel_bb = abs(run.sbv - want_bv) / abs(want_bv), abs(run.sbb - want_bb) / want_bb
    print(f"[{section}] n={v_host.size} L={L} it={run.it} done={run.done} alpha {rel:.2e} alpha_prev {rel_prev:.2e} "
          f"sum bv {rel_bv:.2e} sum bb {rel_bb:.2e} (bar {4 * L * 2.0 ** -53:.2e})")
    assert rel <= 1e-11, (run.alpha, fit["alpha"])
    assert rel_prev <= 1e-11, (run.alpha_prev, fit["alphas"][-1])
    assert rel_bv <= 1e-11, (run.sbv, want_bv)
    assert rel_bb <= 4 * L * 2.0 ** -53, (run.sbb, want_bb)
    for j in range(R.SLOTS):
        for key in ("lo", "hi"):
            g, w = got[key][j], want[key][j]
            assert abs(g - w) <= 1e-11 * abs(w), (key, j, g, w)              # (beyond K: zero, as before the call)
        assert (got["eps"][j], got["eps_n"][j]) == (want["eps"][j], want["eps_n"][j]), j
        if j < want["K"] - 1:
            assert got["lo"][j] == got["hi"][j]                                # one iterate per slot before the last
    return fit


def _hold(section, ops, v_host, L, lo=-1.0, hi=1.0):
    """A row of the table: (a, v_out), held to fp64."""
    run = _call(ops, dev(v_host), None, L, lo=lo, hi=hi)
    assert torch.equal(run.v.view(torch.int32).cpu(), torch.from_numpy(v_host.view(np.int32))), "v_out is not a"
    return run, _check(section, run, v_host, L, lo, hi)


def _table(s):
    return pytest.mark.parametrize("case", F.section(s), ids=lambda c: c.name)


# ------------------------------------------------------------------------------------------------------ a. build paths
@_table("a")
def test_build_paths(ops, case):
    _hold("a paths", ops, F.tensor(case.spec), case.levels)


def test_the_admitted_maximum_is_what_the_table_says(ops):
    assert ops.lib.effq_fp_bucket_max() == F.MAXN
    for n in (1, F.S_MAXN, F.S_MAXN + 1, 262147, F.MAXN):
        assert ops.lib.effq_fp_bucket_ws_bytes(n) == F.workspace_layout(n).total


# ------------------------------------------------------------------------------------------------ b. iteration geometry
@_table("b")
def test_iteration_geometry(ops, case):
    _hold("b geometry", ops, F.tensor(case.spec), case.levels)


# ------------------------------------------------------------------------------ c. boundary segments and integer sums
@_table("c")
def test_boundary_segments_and_integer_sums(ops, case):
    _hold("c segments", ops, F.tensor(case.spec), case.levels)


# ------------------------------------------------------------------------------------------------------------ d. grids
@_table("d")
def test_the_unsigned_grid(ops, case):
    assert (case.lo, case.hi) == (0.0, 1.0)
    _hold("d grids", ops, F.tensor(case.spec), case.levels, lo=0.0, hi=1.0)


# ------------------------------------------------------------------------------------- e. operand modes and alignment
@pytest.mark.parametrize("n", [12001, 36001])
def test_operand_modes_and_alignment(ops, n):
    """(a), (a, v_out) and (a, b, v_out), aligned and with every operand one float off 16-byte alignment: v_out = a + b
    in fp32 bit for bit, and where the values are the same, the same state bits."""
    L = 4
    w, du = R.clustered(n, n), R.normal(n, n + 1, sigma=0.002)
    v = w + du
    runs = []
    for off in (0, 1):
        r_abv = _call(ops, dev(w, off), dev(du, off), L, mode="abv", v_off=off)
        r_av = _call(ops, dev(v, off), None, L, mode="av", v_off=off)
        r_a = _call(ops, dev(v, off), None, L, mode="a")
        for r in (r_abv, r_av):
            assert torch.equal(r.v.view(torch.int32).cpu(), torch.from_numpy(v.view(np.int32))), "v_out is not a + b"
        _check("e modes", r_abv, v, L, -1.0, 1.0)
        runs += [r_abv, r_av, r_a]
    for r in runs[1:]:
        assert r.state_bits == runs[0].state_bits and torch.equal(r.pred_dev[:PRED_CMP], runs[0].pred_dev[:PRED_CMP])


# -------------------------------------------------------------------------------------------------------- f. stop rule
@pytest.mark.parametrize("n", [12000, 36000])
def test_the_cap(ops, n):
    L = 4
    v = R.normal(n, 3 * n + L)
    full = R.iterates(v, L, -1.0, 1.0, TOL, 100 * L)
    assert full["done"] == 1 and full["it"] >= 4 and full["stop_margin"] > 1e-9
    at = _call(ops, dev(v), None, L, max_iter=full["it"])                      # the cap wins although the last step converged
    fit = _check("f stop", at, v, L, -1.0, 1.0, max_iter=full["it"])
    assert (at.done, at.it, fit["alpha"]) == (2, full["it"], full["alpha"])
    after = _call(ops, dev(v), None, L, max_iter=full["it"] + 1)
    _check("f stop", after, v, L, -1.0, 1.0, max_iter=full["it"] + 1)
    assert (after.done, after.it) == (1, full["it"]) and after.state_bits[:4] == at.state_bits[:4]
    one = _call(ops, dev(v), None, L, max_iter=1)
    fit = _check("f stop", one, v, L, -1.0, 1.0, max_iter=1)
    assert (one.done, one.it, one.pred["K"]) == (2, 1, 1) and fit["alpha"] == full["alphas"][1]


@pytest.mark.parametrize("kind", ["zero", "nan", "+inf", "-inf"])
@pytest.mark.parametrize("L", [4, 16])
def test_tensors_without_a_scale(ops, L, kind):
    n = 20001
    x = np.zeros(n, np.float32) if kind == "zero" else R.normal(n, 5)
    if kind != "zero":
        x[n // 3] = np.float32({"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind])
    run = _call(ops, dev(x), None, L)
    fit = _check("f stop", run, x, L, -1.0, 1.0, count_margin=False)
    assert (run.done, run.it, fit["it"], run.pred["K"]) == (2, 0, 0, 0)
    assert torch.equal(run.v.view(torch.int32).cpu(), torch.from_numpy(x.view(np.int32)))


# -------------------------------------------------------------------------------------------------- g. workspace reuse
def test_one_workspace_across_sizes_scales_and_paths(ops):
    L, big = 4, 262147
    base = R.clustered(big, 31)
    seq = [base, R.normal(32769, 32), (base.astype(np.float64) * 100.0).astype(np.float32), R.normal(12000, 33)]
    keep = _workspace(ops.lib, big, 0x00)
    for k, v in enumerate(seq):
        fresh = _once(ops, dev(v), None, L)
        again = _once(ops, dev(v), None, L, ws_keep=keep)
        _same(fresh, again)
        _check("g reuse", again, v, L, -1.0, 1.0)


# ------------------------------------------------------------------------------------------------------------ h. refusals
def test_refusals_leave_everything_untouched(ops):
    lib, L = ops.lib, 4
    n_s, n_g, n_max = 4096, 36000, F.MAXN + 1
    long_a = torch.zeros(n_max, dtype=torch.float32, device=DEV)
    long_a[::7] = 0.25
    a_s, b_s = dev(R.normal(n_s, 1)), dev(R.normal(n_s, 2, sigma=0.01))
    a_g = dev(R.normal(n_g, 3))
    ws_g = lib.effq_fp_bucket_ws_bytes(n_g)
    ws_max = lib.effq_fp_bucket_ws_bytes(F.MAXN) + 8
    # (name, a, b, v_out?, n, levels, lo, hi, max_iter, state?, ws bytes or None for a null workspace, code)
    cases = [("n = 0", a_s, None, True, 0, L, -1.0, 1.0, 400, True, 256, ERR_ARG),
             ("n above the maximum", long_a, None, True, n_max, L, -1.0, 1.0, 400, True, ws_max, ERR_ARG),
             ("one level", a_s, None, True, n_s, 1, -1.0, 1.0, 400, True, 256, ERR_ARG),
             ("257 levels", a_s, None, True, n_s, 257, -1.0, 1.0, 400, True, 256, ERR_ARG),
             ("hi == lo", a_s, None, True, n_s, L, 1.0, 1.0, 400, True, 256, ERR_ARG),
             ("hi < lo", a_s, None, True, n_s, L, 1.0, -1.0, 400, True, 256, ERR_ARG),
             ("max_iter = 0", a_s, None, True, n_s, L, -1.0, 1.0, 0, True, 256, ERR_ARG),
             ("b without v_out", a_s, b_s, False, n_s, L, -1.0, 1.0, 400, True, 256, ERR_ARG),
             ("null a", None, None, True, n_s, L, -1.0, 1.0, 400, True, 256, ERR_ARG),
             ("null state", a_s, None, True, n_s, L, -1.0, 1.0, 400, False, 256, ERR_ARG),
             ("null workspace on the large path", a_g, None, True, n_g, L, -1.0, 1.0, 400, True, None, ERR_ARG),
             ("workspace one byte short", a_g, None, True, n_g, L, -1.0, 1.0, 400, True, ws_g - 1, ERR_WORKSPACE)]
    for name, a, b, with_v, n, levels, lo, hi, max_iter, with_state, wsb, code in cases:
        numel = max(n, 1)
        vbuf, v = _guarded(numel)
        sbuf, st = _bytes_between(40)
        st.fill_(0x3C)
        pbuf, pred = _bytes_between(PRED_BYTES)
        pred.fill_(0x5A)
        ws_buf, ws = _bytes_between(wsb) if wsb is not None else (None, None)
        if ws is not None:
            ws.fill_(0)
        a0, b0 = None if a is None else a.clone(), None if b is None else b.clone()
        rc = lib.effq_fixed_point_bucket_rec(_ptr(a), _ptr(b), _ptr(v) if with_v else None, n, levels, lo, hi, TOL, max_iter,
                                             _ptr(st) if with_state else None, _ptr(ws), 0 if wsb is None else wsb, _ptr(pred),
                                             ops.stream)
        torch.cuda.synchronize()
        assert rc == code, (name, rc)
        assert bool((st == 0x3C).all()) and bool((pred == 0x5A).all()) and bool(torch.isnan(v).all()), name
        assert _bytes_untouched(sbuf) and _bytes_untouched(pbuf) and _guards_untouched(vbuf, numel), name
        assert ws is None or (not bool(ws.any()) and _bytes_untouched(ws_buf)), name
        assert a is None or torch.equal(a, a0), name
        assert b is None or torch.equal(b, b0), name
