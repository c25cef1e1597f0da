"""effq_fixed_point_traj and effq_fixed_point_traj_parts (csrc/fixed_point_traj.hip, csrc/fp_traj.h, the recorder of
csrc/fp_level.h) class by class against the fp64 restatement of tests/fp_traj_ref.py (-m gpu).

Phase 2 of the kernel serves an iterate in one of five ways: from the first wave's registers (narrow list <= 1024), from the
workgroup's registers (<= 4096), from the streamed narrow list, from both lists (the iterate left its narrow bracket) or by
a full pass (it left the wide one, or the call is cold) - vectorised where v_out is 16-byte aligned, scalar otherwise.  A
case here first derives, from the prediction as read from the device, the way every iterate must be served and how many
values phase 1 must list (fp_traj_ref.classify), asserts after the call that the kernel's own counters moved by exactly
that, and then holds the result to fp64: equal iteration count, alpha within 1e-11, within 1e-13 of the bucketed kernel.

  a. sizes from one value to the admitted 2^23, both sides of the 4096 values of a workgroup, 2 / 3 / 4 / 16 levels, the
     unsigned grid, the refusals, the three ways of reaching the values of a full pass;
  b. the seven-call schedule of fp_traj_ref.SCHEDULE: every way above, the recorder's new prediction against
     fp_traj_ref.record;
  c. values on level boundaries of the iterates, zeros, denormals, duplicates, an outlier, constant tensors; zero and
     non-finite tensors against the bucketed kernel;
  d. the iteration cap in the full-pass, the one-wave and the workgroup loop;
  e. predictions that are garbage: bytes, an impossible K, and a tensor's own record with one field no call would have
     recorded (a unit too coarse or infinite, a narrow bracket outside its wide one, a bracket across zero);
  f. the K-slice prologue at ragged shapes against the slices summed on the host.

Every call runs inside sentinel bands (outputs NaN-prefilled, between 64-float guards; state, prediction and a workspace
of exactly effq_fp_traj_ws_bytes(n) bytes between guards), once on a workspace filled with 0xFF behind its zero header and
once on a zero-filled one: equal bits, guards untouched, header counters back to zero."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

from tests import fp_traj_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                       # floats on either side of an output (keeps the output 256-byte aligned)
SENTINEL = -7.25e33
BYTE = 0xA5                      # guard bytes around the workspace, the state and the prediction
TOL = 1e-5
PRED_BYTES = 16 + 8 * 63
PRED_CMP = 16 + 8 * 55           # everything before the time stamps
ERR_ARG, ERR_WORKSPACE = 1, 3
COUNTERS = ("listed", "ring_listed", "warm_iters", "ring_iters", "full_iters")
WORST = {}                       # section -> worst relative deviation of alpha seen (printed when the module ends)


@pytest.fixture(scope="module")
def ops():
    from efficientq_amd.hip_ops import get_ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert get_ops(DEV).lib.effq_fp_traj_pred_bytes() == PRED_BYTES
    t0 = time.time()
    yield get_ops(DEV)
    print(f"\ntest_fp_traj_classes_gpu: {time.time() - t0:.1f} s; worst |alpha - ref| / ref per section: "
          + ", ".join(f"{k}: {v:.2e}" for k, v in sorted(WORST.items())))


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _note(section, got, want):
    rel = abs(got - want) / abs(want)
    WORST[section] = max(WORST.get(section, 0.0), rel)
    return rel


def _guarded(numel, offset=0):
    """A NaN-filled device vector inside a sentinel-filled buffer; `offset` floats off the 256-byte alignment."""
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


class Run:
    pass


def _once(ops, a, b, L, pred, fill, lo, hi, max_iter, v_mode, ws_keep=None):
    lib, n = ops.lib, a.numel()
    r = Run()
    wsb = lib.effq_fp_traj_ws_bytes(n)
    if ws_keep is None:
        r.ws_buf, r.ws = _bytes_between(wsb)
        r.ws[:256] = 0                                   # the header contract
        r.ws[256:] = fill
    else:
        r.ws_buf, r.ws = ws_keep
    off = {"aligned": 0, "offset": 1, "null": 0}[v_mode]
    vbuf, v = _guarded(n, off) if v_mode != "null" else (None, None)
    sbuf, sview = _bytes_between(40)
    sview.fill_(0xFF)
    pbuf, pview = _bytes_between(PRED_BYTES)
    pview.copy_(pred)
    rc = lib.effq_fixed_point_traj(_ptr(a), _ptr(b), _ptr(v), n, L, lo, hi, TOL, max_iter, _ptr(sview), _ptr(pview),
                                   _ptr(r.ws), wsb, ops.stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _bytes_untouched(r.ws_buf), "wrote outside the workspace"
    assert _bytes_untouched(sbuf), "wrote outside the state"
    assert _bytes_untouched(pbuf), "wrote outside the prediction"
    assert v is None or _guards_untouched(vbuf, n, off), "wrote outside v_out"
    assert r.ws[:12].view(torch.int32).tolist() == [0, 0, 0], "header counters not back to zero"
    st = sview.clone().view(torch.float64)
    r.state_bits = st.view(torch.int64).cpu().tolist()
    r.alpha, r.it, r.done = ops.read_fp_state(st)
    r.pred_dev = pview.clone()
    r.pred = ops.read_fp_pred(r.pred_dev)
    r.v = v
    return r


def _call(ops, a, b, L, pred, lo=-1.0, hi=1.0, max_iter=None, v_mode="aligned"):
    """One call from a copy of `pred` on a workspace poisoned with 0xFF and one on zeros: equal bits.  -> Run"""
    max_iter = 100 * L if max_iter is None else max_iter
    r1 = _once(ops, a, b, L, pred, 0xFF, lo, hi, max_iter, v_mode)
    r2 = _once(ops, a, b, L, pred, 0x00, lo, hi, max_iter, v_mode)
    assert r1.state_bits == r2.state_bits, "the result depends on stale workspace contents"
    assert torch.equal(r1.pred_dev[:PRED_CMP], r2.pred_dev[:PRED_CMP])
    if r1.v is not None:
        assert torch.equal(r1.v.view(torch.int32), r2.v.view(torch.int32))
    return r1


def _bucket(ops, a, b, L, lo=-1.0, hi=1.0, max_iter=None):
    """(alpha, iters, done) of effq_fixed_point_bucket on the same operands."""
    lib, n = ops.lib, a.numel()
    ws = ops._workspace("fp_bucket", lib.effq_fp_bucket_ws_bytes(n))
    st, v = ops.new_fp_state(), torch.empty(n, device=DEV)
    rc = lib.effq_fixed_point_bucket(_ptr(a), _ptr(b), _ptr(v), n, L, lo, hi, TOL, 100 * L if max_iter is None else max_iter,
                                     _ptr(st), _ptr(ws), ws.numel(), ops.stream)
    assert rc == 0
    return ops.read_fp_state(st)


def _delta(before, after):
    return {k: after[k] - before[k] for k in COUNTERS}


def _expect(cls):
    c = cls["classes"]
    return {"listed": cls["m_n"], "ring_listed": cls["m_r"], "warm_iters": c.count("n"), "ring_iters": c.count("r"),
            "full_iters": c.count("f")}


def _hold(section, ops, a, b, v_host, L, pred_dev, lo=-1.0, hi=1.0, bucket=True, v_mode="aligned", check_record=False,
          defer_bucket=False):
    """One guarded call held to the restatement: the class first, then the bars.  -> (Run, fit, cls)
    defer_bucket: the caller asserts run.vs_bucket <= 1e-13 itself, after the calls that follow."""
    before = ops.read_fp_pred(pred_dev)
    fit = R.iterates(v_host, L, lo, hi, TOL, 100 * L)
    assert fit["stop_margin"] > 1e-9, "the case's stop decision is a coin toss: choose another tensor"
    cls = R.classify(before, v_host, L, lo, hi, fit["alphas"])
    run = _call(ops, a, b, L, pred_dev, lo, hi, v_mode=v_mode)
    rel = _note(section, run.alpha, fit["alpha"]) if fit["done"] == 1 else float("nan")
    if fit["done"] == 1:
        _note(f"levels {L:2d}", run.alpha, fit["alpha"])
    print(f"[{section}] n={v_host.size} L={L} it={run.it}/{fit['it']} m_n={cls['m_n']} m_r={cls['m_r']} "
          f"classes={cls['classes'][:24]} counters={_delta(before, run.pred)} rel={rel:.2e}")
    assert _delta(before, run.pred) == _expect(cls), (_delta(before, run.pred), _expect(cls), cls["classes"])
    if run.v is not None:
        assert torch.equal(run.v.view(torch.int32).cpu(), torch.from_numpy(v_host.view(np.int32))), "v_out is not a + b"
    assert (run.done, run.it) == (fit["done"], fit["it"]), (run.done, run.it, fit["done"], fit["it"])
    if fit["done"] == 1:
        assert rel <= 1e-11, (run.alpha, fit["alpha"])
    assert run.pred["calls"] == before["calls"] + 1
    if check_record:
        want = R.record(before, fit["alphas"], fit["alpha"], fit["sum_abs"], L)
        got = run.pred
        assert (got["K"], got["e"], got["e_valid"]) == (want["K"], want["e"], want["e_valid"])
        for j in range(R.SLOTS):
            for key, bar in (("lo", 1e-12), ("hi", 1e-12), ("eps", 1e-6), ("eps_n", 1e-6)):
                g, w = got[key][j], want[key][j]
                if j < want["K"]:
                    assert abs(g - w) <= bar * abs(w), (key, j, g, w)
                else:
                    assert g == before[key][j], (key, j)                          # untouched beyond the new K
    if bucket:                                       # (last: every check above has then been made)
        ab, ib, db = _bucket(ops, a, b, L, lo, hi)
        assert (db, ib) == (run.done, run.it)
        if fit["done"] == 1:
            run.vs_bucket = _note(section + " vs bucket", run.alpha, ab)
            print(f"[{section}] n={v_host.size} L={L} bucketed kernel: vs this {run.vs_bucket:.2e}, vs fp64 "
                  f"{abs(ab - fit['alpha']) / fit['alpha']:.2e}")
            assert defer_bucket or run.vs_bucket <= 1e-13, (run.alpha, ab)
    return run, fit, cls


# ------------------------------------------------------------------------------------------------------------ a. sizes
def _sized(n, L, lo=-1.0):
    w, du = R.normal(n, 7 * n + L), R.normal(n, 11 * n + L, sigma=0.01)
    if lo == 0.0:
        w, du = np.maximum(w, np.float32(0)), np.abs(du) * (w > 0)                # post-ReLU: exact zeros, no negatives
    return w, du.astype(np.float32)


def _cold_then_warm(section, ops, w, du, L, lo=-1.0, bucket=True):
    pred = ops.new_fp_pred()
    run, fit, cls = _hold(section, ops, dev(w), dev(du), w + du, L, pred, lo=lo, bucket=bucket)
    assert set(cls["classes"]) == {"f"} and run.pred["K"] == min(fit["it"], 8) and run.pred["listed"] == 0
    w2, du2 = (w.astype(np.float64) * 1.0005).astype(np.float32), (du.astype(np.float64) * 1.0005).astype(np.float32)
    run2, fit2, cls2 = _hold(section, ops, dev(w2), dev(du2), w2 + du2, L, run.pred_dev, lo=lo, bucket=bucket)
    assert cls2["warm"] and cls2["tallies_ok"]


@pytest.mark.parametrize("L", [2, 3, 4, 16])
@pytest.mark.parametrize("n", [1, 2, 63, 511, 4095, 4096, 4097, 8191 + 4096, 65536, 65541, 262149])
def test_sizes_cold_and_warm(ops, n, L):
    _cold_then_warm("a sizes", ops, *_sized(n, L), L)


def test_the_admitted_maximum(ops):
    n = R.MAXN
    assert ops.lib.effq_fp_traj_max() == n
    w = R.clustered(n, 23)
    du = np.resize(R.normal(1 << 20, 24, sigma=0.002), n)
    _cold_then_warm("a sizes", ops, w, du, 4)


def test_the_unsigned_grid(ops):
    _cold_then_warm("a sizes", ops, *_sized(65541, 4, lo=0.0), 4, lo=0.0)


def test_refusals_leave_everything_untouched(ops):
    lib, n, L = ops.lib, 4096, 4
    a, b = dev(R.normal(n, 1)), dev(R.normal(n, 2, sigma=0.01))
    wsb = lib.effq_fp_traj_ws_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    cases = [("n above the maximum", a, b, "v", R.MAXN + 1, wsb, ERR_ARG),
             ("workspace one byte short", a, b, "v", n, wsb - 1, ERR_WORKSPACE),
             ("v_out == a", a, b, "a", n, wsb, ERR_ARG), ("v_out == b", a, b, "b", n, wsb, ERR_ARG),
             ("b without v_out", a, b, None, n, wsb, ERR_ARG)]
    for name, pa, pb, vsel, nn, nbytes, code in cases:
        vbuf, v = _guarded(n)
        st = torch.full((5,), float("nan"), dtype=torch.float64, device=DEV)
        pred = torch.full((PRED_BYTES,), 0x5A, dtype=torch.uint8, device=DEV)
        a0, b0 = a.clone(), b.clone()
        vp = {"v": v, "a": pa, "b": pb, None: None}[vsel]
        rc = lib.effq_fixed_point_traj(_ptr(pa), _ptr(pb), _ptr(vp), nn, L, -1.0, 1.0, TOL, 400, _ptr(st), _ptr(pred), _ptr(ws),
                                       nbytes, ops.stream)
        torch.cuda.synchronize()
        assert rc == code, (name, rc)
        assert bool(torch.isnan(st).all()) and bool((pred == 0x5A).all()) and bool(torch.isnan(v).all()), name
        assert torch.equal(a, a0) and torch.equal(b, b0) and not bool(ws.any()), name


@pytest.mark.parametrize("n", [12288, 12289, 12290, 12291])
def test_the_three_ways_to_the_values_of_a_full_pass(ops, n):
    """v_out 16-byte aligned (float4 loads and a scalar tail of n % 4), v_out 4 bytes off (scalar), no v_out (scalar, from
    a): the same state in bits, cold (every iterate a full pass) and past the wide bracket of a warm call."""
    L = 4
    w, du = R.clustered(n, n), R.normal(n, n + 1, sigma=0.002)
    v = w + du
    big = (v.astype(np.float64) * 1.2).astype(np.float32)
    cold = ops.new_fp_pred()
    runs = [_hold("a sizes", ops, dev(w), dev(du), v, L, cold, v_mode="aligned")[0],
            _hold("a sizes", ops, dev(w), dev(du), v, L, cold, v_mode="offset", bucket=False)[0],
            _hold("a sizes", ops, dev(v), None, v, L, cold, v_mode="null", bucket=False)[0]]
    assert runs[0].state_bits == runs[1].state_bits == runs[2].state_bits
    assert torch.equal(runs[0].pred_dev[:PRED_CMP], runs[1].pred_dev[:PRED_CMP])
    assert torch.equal(runs[0].pred_dev[:PRED_CMP], runs[2].pred_dev[:PRED_CMP])
    warm = []
    for mode in ("aligned", "offset", "null"):
        run, fit, cls = _hold("a sizes", ops, dev(big), None, big, L, runs[0].pred_dev, v_mode=mode,
                              bucket=mode == "aligned")
        assert set(cls["classes"]) == {"f"} and cls["warm"] and cls["tallies_ok"]
        warm.append(run)
    assert warm[0].state_bits == warm[1].state_bits == warm[2].state_bits


# ------------------------------------------------------------------------------------------------- b. dispatch classes
@functools.lru_cache(maxsize=None)
def _walk(case):
    """The schedule of `case` through the restatement alone: [(v, fit, cls)] per call."""
    n, L, kind = case
    base, pred, calls = R.schedule_base(n, L, kind), R.cold_pred(), []
    for k in range(len(R.SCHEDULE)):
        v = R.scheduled(base, k)
        fit = R.iterates(v, L, -1.0, 1.0, TOL, 100 * L)
        cls = R.classify(pred, v, L, -1.0, 1.0, fit["alphas"])
        calls.append((v, fit, cls))
        pred = R.record(pred, fit["alphas"], fit["alpha"], fit["sum_abs"], L)
    return calls


@pytest.mark.parametrize("case", R.SCHEDULE_CASES, ids=lambda c: f"{c[0]}-L{c[1]}")
def test_schedule_runs_the_classes_it_was_built_for(ops, case):
    n, L, _ = case
    pred = ops.new_fp_pred()
    for k, (v, fit_ref, cls_ref) in enumerate(_walk(case)):
        # (the class is derived from the prediction the DEVICE holds; the walk above only says what the case is for)
        run, fit, cls = _hold("b classes", ops, dev(v), None, v, L, pred, check_record=True)
        assert cls["bracket_margin"] > 1e-9
        assert R.reached(cls, fit["it"]) == R.reached(cls_ref, fit_ref["it"]), (k, cls, cls_ref)
        assert (cls["m_n"], cls["m_r"], cls["classes"]) == (cls_ref["m_n"], cls_ref["m_r"], cls_ref["classes"]), k
        again = _once(ops, dev(v), None, L, pred, 0xFF, -1.0, 1.0, 100 * L, "aligned")      # from the same prediction
        assert again.state_bits == run.state_bits and torch.equal(again.pred_dev[:PRED_CMP], run.pred_dev[:PRED_CMP])
        pred = run.pred_dev


def test_the_schedules_cover_every_class():
    got = set()
    for case in R.SCHEDULE_CASES:
        for _, fit, cls in _walk(case):
            got |= R.reached(cls, fit["it"])
    assert got == set(R.REQUIRED), set(R.REQUIRED) - got


# ------------------------------------------------------------------------------------------------ c. adversarial values
@functools.lru_cache(maxsize=None)
def _adversarial(L):
    return R.adversarial(L)


@pytest.mark.parametrize("big", [False, True], ids=["alone", "appended"])
@pytest.mark.parametrize("name", ["boundaries", "zeros_tiny", "duplicates", "outlier", "all_equal", "two_values"])
@pytest.mark.parametrize("L", [2, 3, 4, 5, 16])
def test_adversarial_values_cold_and_twice_warm(ops, L, name, big):
    """[2-outlier-alone] and [4-outlier-alone] are a finding of this file about the OTHER kernel: with one value of 500
    among 20 000 of ~0.1 effq_fixed_point_bucket ended 2.2e-13 and 1.0e-13 from fp64 (this kernel: 0 and 6e-16), because
    its integer unit was a fixed fraction of a bucket width that the outlier stretches; k_fps now refines the unit by the
    ratio max|v| / mean|v| (fixed_point_bucket.hip)."""
    x = _adversarial(L)[name]
    if big:
        x = np.concatenate([x, R.normal(65536, 77 + L, sigma=0.1)])
    pred, vs_bucket = ops.new_fp_pred(), []
    for k, m in enumerate((1.0, 1.0 + 1e-4, 1.0 + 1e-4 + 1e-6)):
        v = (x.astype(np.float64) * m).astype(np.float32)
        run, fit, cls = _hold("c adversarial", ops, dev(v), None, v, L, pred, check_record=True, defer_bucket=True)
        assert set(cls["classes"]) == ({"f"} if k == 0 else {"n"})
        vs_bucket.append(run.vs_bucket)
        pred = run.pred_dev
    assert max(vs_bucket) <= 1e-13, vs_bucket


def _same_bits_or_both_nan(x, y):
    return (np.isnan(x) and np.isnan(y)) or np.float64(x).view(np.int64) == np.float64(y).view(np.int64)


@pytest.mark.parametrize("kind", ["zero", "nan", "inf"])
@pytest.mark.parametrize("L", [2, 4, 16])
def test_tensors_without_a_scale_end_as_the_bucketed_kernel_does(ops, L, kind):
    """An all-zero tensor, one NaN, one Inf: there is no fp64 answer; the trajectory kernel must hand the loop the same
    (done, iters, alpha) as the kernel it takes over from, cold and from the prediction of a finite tensor."""
    n = 20001
    good = R.normal(n, 5)
    x = np.zeros(n, np.float32) if kind == "zero" else good.copy()
    if kind != "zero":
        x[n // 3] = np.float32(np.nan if kind == "nan" else np.inf)
    warm = _call(ops, dev(good), None, L, ops.new_fp_pred()).pred_dev
    ab, ib, db = _bucket(ops, dev(x), None, L)
    for pred in (ops.new_fp_pred(), warm):
        run = _call(ops, dev(x), None, L, pred)
        print(f"[c no scale] {kind} L={L}: traj {(run.done, run.it, run.alpha)} bucket {(db, ib, ab)}")
        assert (run.done, run.it) == (db, ib) and _same_bits_or_both_nan(run.alpha, ab), (run.alpha, ab)


# ------------------------------------------------------------------------------------------------------------- d. cap
@pytest.mark.parametrize("n,way", [(32773, "one wave"), (65541, "workgroup")])
def test_the_cap_in_every_loop(ops, n, way):
    L, cap = 4, 3
    v = R.clustered(n, 2)
    v2 = R.scheduled(v, 1)
    full, full2 = R.iterates(v, L, -1.0, 1.0, TOL, 400), R.iterates(v2, L, -1.0, 1.0, TOL, 400)
    assert full["it"] == 6 and full2["it"] == 6              # the cap of 3 lands three steps before convergence
    assert min(full["stop_margin"], full2["stop_margin"]) > 1e-9
    # cold: the cap in the full-pass loop; the next call on the SAME workspace (no refill) is correct
    r = _once(ops, dev(v), None, L, ops.new_fp_pred(), 0xFF, -1.0, 1.0, cap, "aligned")
    assert (r.done, r.it) == (2, cap) and _note("d cap", r.alpha, full["alphas"][cap]) <= 1e-11
    assert r.pred["full_iters"] == cap and r.pred["K"] == cap
    nxt = _once(ops, dev(v), None, L, ops.new_fp_pred(), None, -1.0, 1.0, 400, "aligned", ws_keep=(r.ws_buf, r.ws))
    assert (nxt.done, nxt.it) == (1, full["it"]) and _note("d cap", nxt.alpha, full["alpha"]) <= 1e-11
    # warm: the cap in the loop of the first wave (narrow list <= 1024) / of the workgroup
    cls = R.classify(nxt.pred, v2, L, -1.0, 1.0, full2["alphas"])
    assert set(cls["classes"]) == {"n"} and (cls["m_n"] <= R.ONE_WAVE_MAX) == (way == "one wave"), cls
    r2 = _once(ops, dev(v2), None, L, nxt.pred_dev, 0xFF, -1.0, 1.0, cap, "aligned", ws_keep=(nxt.ws_buf, nxt.ws))
    assert (r2.done, r2.it) == (2, cap) and _note("d cap", r2.alpha, full2["alphas"][cap]) <= 1e-11
    assert r2.pred["warm_iters"] - nxt.pred["warm_iters"] == cap and r2.pred["listed"] - nxt.pred["listed"] == cls["m_n"]
    r3 = _once(ops, dev(v2), None, L, r2.pred_dev, None, -1.0, 1.0, 400, "aligned", ws_keep=(r2.ws_buf, r2.ws))
    assert (r3.done, r3.it) == (1, full2["it"]) and _note("d cap", r3.alpha, full2["alpha"]) <= 1e-11


# ------------------------------------------------------------------------------------------- e. untrusted predictions
def _garbage(ops, kind, other_pred, own_pred):
    if kind == "0xFF":
        return torch.full((PRED_BYTES,), 0xFF, dtype=torch.uint8, device=DEV)
    if kind.startswith("random"):
        return dev(np.random.default_rng(int(kind[6:])).integers(0, 256, PRED_BYTES, dtype=np.uint8))
    if kind in ("K=9", "K=-3"):
        p = other_pred.clone()
        p[:4].view(torch.int32)[0] = 9 if kind == "K=9" else -3
        return p
    # the tensor's OWN record (every iterate lands inside its brackets) with one field that no call would have recorded
    p = own_pred.clone()
    i32, f64 = p[:16].view(torch.int32), p[16:16 + 8 * 40].view(torch.float64)
    if kind == "unit 2^40 too coarse":
        i32[1] -= 40
    elif kind == "unit 2^-2000000000":
        i32[1] = -2000000000
    elif kind == "negative wide margin":           # the narrow bracket then lies outside the wide one
        f64[16:24] = -0.5
    elif kind == "negative lo":                    # a bracket across zero: the level is not monotone over it
        f64[0:8] = -f64[0:8]
    else:
        raise ValueError(kind)
    return p


@pytest.mark.parametrize("kind", ["0xFF", "random1", "random2", "random3", "K=9", "K=-3", "unit 2^40 too coarse",
                                  "unit 2^-2000000000", "negative wide margin", "negative lo"])
@pytest.mark.parametrize("n,L", [(4095, 4), (65541, 4), (65541, 16)])
def test_untrusted_predictions_cost_nothing_but_speed(ops, n, L, kind):
    """random1 is a finding of this file: K clamps to 8, e = -2.1e9 made the unit 2^-e infinite and passed the overflow
    test, slot 0 held a narrow bracket [7.7e-127, 5.3e8] outside its wide one, which the first wave alone does not look at:
    alpha = NaN after one iteration.  The last four kinds are that prediction's defects one at a time."""
    v = R.clustered(n, 3 * n + L)
    cold = _call(ops, dev(v), None, L, ops.new_fp_pred())
    other = _call(ops, dev(R.clustered(n, 5 * n + L, alpha=0.0703)), None, L, ops.new_fp_pred()).pred_dev
    run = _call(ops, dev(v), None, L, _garbage(ops, kind, other, cold.pred_dev))
    print(f"[e untrusted] n={n} L={L} {kind}: it={run.it}/{cold.it} rel={_note('e untrusted', run.alpha, cold.alpha):.2e}")
    assert (run.done, run.it) == (cold.done, cold.it)
    assert abs(run.alpha - cold.alpha) <= 1e-13 * cold.alpha, (run.alpha, cold.alpha)


# ------------------------------------------------------------------------------------------------------- f. K slices
def _parts_fn(lib):
    fn = lib.effq_fixed_point_traj_parts
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                   C.c_void_p]
    return fn


@pytest.mark.parametrize("c2,nwrow,has_b,nsplit,ldp", [(80, 867, 1, 2, 896), (80, 867, 0, 1, 867), (512, 128, 1, 3, 160),
                                                       (512, 129, 1, 2, 130), (3, 21846, 0, 5, 21856)])
def test_k_slices_at_ragged_shapes(ops, c2, nwrow, has_b, nsplit, ldp):
    """w*, b*, v and the state bit-identical to the slices summed in slice order on the host and effq_fixed_point_traj on
    the sum, cold and warm, where c2 * nwrow is no multiple of a workgroup's 4096 values (the n - 1 clamp, the row / column
    split of the last workgroup), at c2 = 512 (the width of the bias prologue) and with one slice."""
    lib, fn, L = ops.lib, _parts_fn(ops.lib), 4
    n = c2 * nwrow
    rng = np.random.default_rng(c2 * 1000 + nwrow)
    w = R.clustered(n, n).reshape(c2, nwrow)
    du = R.normal(n, n + 1, sigma=0.002)
    pred_a, pred_b = ops.new_fp_pred(), ops.new_fp_pred()
    for rep in range(2):
        w = (w.astype(np.float64) * (1.0 + 2e-4 * rep)).astype(np.float32)
        parts = (0.01 * rng.standard_normal((nsplit, c2, ldp))).astype(np.float32)     # padding columns hold noise too
        rest = parts[1:].sum(0, dtype=np.float32) if nsplit > 1 else np.zeros((c2, ldp), np.float32)
        parts[0, :, :nwrow] = w - rest[:, :nwrow]
        acc = parts[0].copy()
        for z in range(1, nsplit):
            acc = acc + parts[z]                                                   # fp32, slice order
        w_sum = np.ascontiguousarray(acc[:, :nwrow]).reshape(-1)
        b_sum = np.ascontiguousarray(acc[:, nwrow]) if has_b else None
        v_host = w_sum + du
        ref, fit, cls = _hold("f slices", ops, dev(w_sum), dev(du), v_host, L, pred_a, bucket=False)
        assert set(cls["classes"]) == ({"f"} if rep == 0 else {"n"})
        parts_d, du_d = dev(parts), dev(du)
        for fill in (0xFF, 0x00):
            ws_buf, ws = _bytes_between(lib.effq_fp_traj_ws_bytes(n))
            ws[:256] = 0
            ws[256:] = fill
            wbuf, wst = _guarded(n)
            bbuf, bst = _guarded(c2) if has_b else (None, None)
            vbuf, v = _guarded(n)
            sbuf, st = _bytes_between(40)
            pbuf, pv = _bytes_between(PRED_BYTES)
            pv.copy_(pred_b)
            rc = fn(parts_d.data_ptr(), nsplit, ldp, c2, nwrow, has_b, du_d.data_ptr(), wst.data_ptr(),
                    bst.data_ptr() if has_b else None, v.data_ptr(), L, -1.0, 1.0, TOL, 100 * L, st.data_ptr(), pv.data_ptr(),
                    ws.data_ptr(), ws.numel(), ops.stream)
            assert rc == 0
            torch.cuda.synchronize()
            assert _guards_untouched(wbuf, n) and _guards_untouched(vbuf, n) and (bbuf is None or _guards_untouched(bbuf, c2))
            assert _bytes_untouched(ws_buf) and _bytes_untouched(sbuf) and _bytes_untouched(pbuf)
            assert ws[:12].view(torch.int32).tolist() == [0, 0, 0]
            assert torch.equal(wst.view(torch.int32).cpu(), torch.from_numpy(w_sum.view(np.int32)))
            assert torch.equal(v.view(torch.int32).cpu(), torch.from_numpy(v_host.view(np.int32)))
            if has_b:
                assert torch.equal(bst.view(torch.int32).cpu(), torch.from_numpy(b_sum.view(np.int32)))
            assert st.clone().view(torch.int64).cpu().tolist() == ref.state_bits
            assert torch.equal(pv[:PRED_CMP], ref.pred_dev[:PRED_CMP])
        pred_a, pred_b = ref.pred_dev, pv.clone()


def test_more_rows_than_the_bias_prologue_has_threads_is_refused(ops):
    fn, n = _parts_fn(ops.lib), 513 * 8
    part, du = torch.zeros(513 * 16, device=DEV), torch.zeros(n, device=DEV)
    wst, bst, v = (torch.full((n,), float("nan"), device=DEV) for _ in range(3))
    st, pred = ops.new_fp_state(), ops.new_fp_pred()
    ws = torch.zeros(ops.lib.effq_fp_traj_ws_bytes(n), dtype=torch.uint8, device=DEV)
    rc = fn(part.data_ptr(), 1, 16, 513, 8, 1, du.data_ptr(), wst.data_ptr(), bst.data_ptr(), v.data_ptr(), 4, -1.0, 1.0, TOL,
            400, st.data_ptr(), pred.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream)
    torch.cuda.synchronize()
    assert rc == ERR_ARG
    assert bool(torch.isnan(wst).all()) and bool(torch.isnan(bst).all()) and bool(torch.isnan(v).all())
    assert not bool(st.any()) and not bool(pred.any()) and not bool(ws.any())
