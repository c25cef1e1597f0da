"""The choice of kernels of one layer's calibration (qconv.layer_paths / LayerPaths) as a value: against a frozen
restatement of the conditions EfficientQConvHIP.ptq held inline before the choice became a function, as literal rows for
the layer classes the code comments speak of, and through the sequence of ops calls one small layer issues."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from tests import cpu_backend

MAX_N, I8_MAX_N = 1729, 8000        # qconv.GRAM_LOSS_MAX_N, qconv.GRAM_LOSS_I8_MAX_N when the specification was frozen
CAPS = ("conv_i8_supported", "conv_i8s_supported", "gram_i8_supported", "gram_loss", "gram_loss_i8_supported",
        "gram_f64_supported", "conv_i8_out_supported")


def _stub(**answers):
    """An ops object that only answers the capability questions: each *_supported(...) with a fixed yes / no; `gram_loss`
    (asked for by presence) is there or is not."""
    ops = SimpleNamespace()
    for name in CAPS:
        if name == "gram_loss":
            if answers.get(name, False):
                ops.gram_loss = lambda *a: None
        else:
            setattr(ops, name, lambda *a, _yes=bool(answers.get(name, False)): _yes)
    return ops


ALL = {name: True for name in CAPS}


def frozen_specification(ops, geom, self, has_b, c2, n_sys, voxels, GRAM_LOSS_DEFAULT, att_ok, planes_ok):
    """FROZEN: the boolean expressions of EfficientQConvHIP.ptq as they stood inline (commit 8d13108), copied once, in
    their order, with GRAM_LOSS_MAX_N / GRAM_LOSS_I8_MAX_N at their values of that commit.  What the method did between
    them is reduced to its effect on them: `att_ok` = att_classes() returned classes, `planes_ok` = gram_loss_i8_planes()
    returned planes, `xidx is not None` = level ids were asked for (quant_dequant_f64path returns them exactly then).
    Do not edit: the function under test is compared with THIS."""
    GRAM_LOSS_MAX_N, GRAM_LOSS_I8_MAX_N = MAX_N, I8_MAX_N
    use_i8 = bool(self.q_act and not self._act_inited and self.lwq_exact_int and
                  getattr(ops, "conv_i8_supported", lambda *a: False)(geom, self.qlvl_act, self.qlvl_w))
    use_i8s = bool((not use_i8) and self.q_act and not self._act_inited and self.lwq_exact_int and
                   getattr(ops, "conv_i8s_supported", lambda *a: False)(geom, self.qlvl_act, self.qlvl_w))
    int_conv = use_i8 or use_i8s
    use_gi8 = bool(self.q_act and not self._act_inited and self.lwq_exact_int and
                   getattr(ops, "gram_i8_supported", lambda *a: False)(geom, self.qlvl_act))
    chan = self.channel_wise
    if chan:
        use_i8 = use_i8s = int_conv = False
    att_cls = (object() if att_ok else None) if use_gi8 else None
    use_gi8 = att_cls is not None
    want_idx = xidx = None
    if self.q_act:
        if self._act_inited:
            pass
        else:
            want_idx = int_conv or use_gi8
            xidx = object() if want_idx else None
    loss_gram = None
    gram_call = None
    use_gl = bool(use_gi8 and GRAM_LOSS_DEFAULT and hasattr(ops, "gram_loss") and n_sys <= GRAM_LOSS_MAX_N and
                  voxels >= 8 * n_sys)
    use_gl8 = bool(use_gi8 and GRAM_LOSS_DEFAULT and not use_gl and not chan and
                   GRAM_LOSS_MAX_N < n_sys <= GRAM_LOSS_I8_MAX_N and
                   getattr(ops, "gram_loss_i8_supported", lambda *a: False)(c2, n_sys, has_b, self.qlvl_w))
    if use_gi8 and (use_gl or use_gl8):
        gram_call = "gram_i8(unweighted)"
        loss_gram = ("Au", "Bu", "syy")
        if use_gl8:
            planes = object() if planes_ok else None
            loss_gram = ("Au", "Bu", "syy", planes) if planes is not None else None
    elif use_gi8:
        gram_call = "gram_i8"
    else:
        gram_call = "gram"
        if (not self.q_act and GRAM_LOSS_DEFAULT and self.lwq_exact_int and n_sys <= GRAM_LOSS_MAX_N and
                voxels >= 8 * n_sys and
                getattr(ops, "gram_f64_supported", lambda *a: False)(geom, has_b)):
            loss_gram = ("Au_f64", "Bu_f64", "syy")
    loss_kind = 1 if use_i8 else (2 if use_i8s else 0)
    fuse = self.q_act and not self._act_inited
    fwd_i8 = bool(fuse and xidx is not None and self.lwq_exact_int and not chan and
                  getattr(ops, "conv_i8_out_supported", lambda *a: False)(geom, self.qlvl_act, self.qlvl_w))
    return dict(loss_kind=loss_kind, gram_call=gram_call, loss_gram=loss_gram, want_idx=want_idx, fwd_i8=fwd_i8,
                exact_int=int_conv or loss_gram is not None, exact_gram=use_gi8)


def _effects(p):
    """What a final LayerPaths makes ptq do, in the terms of frozen_specification's result."""
    loss_gram = {None: None, "gram_f64": ("Au", "Bu", "syy"), "gram_f64_fp_input": ("Au_f64", "Bu_f64", "syy")}.get(p.losses)
    if p.losses == "gram_i8":
        loss_gram = "four"
    return dict(loss_kind=p.loss_kind, loss_gram=loss_gram, want_idx=p.want_idx, fwd_i8=p.fwd_i8,
                exact_int=p.conv is not None or p.losses is not None, exact_gram=p.gram_i8)


def test_layer_paths_equal_the_frozen_specification_on_the_full_cross_product():
    """Every flag x every capability answer x gram_loss_enabled x n_sys x voxels x att_classes_ok x planes_ok: the paths
    the function chooses (and after() adjusts) make ptq do what the frozen conditions made it do.  The Gram call is
    derived as ptq derives it: the unweighted integer call where the paths BEFORE the planes are known want losses from
    the integer Gram system."""
    import efficientq_amd.qconv as Q
    geom = object()
    n_cases = 0
    flags = list(itertools.product((False, True), repeat=4))
    sizes = [(n, v) for n in (1728, 1729, 1730, 8000, 8001) for v in (8 * n - 1, 8 * n)]
    for caps in itertools.product((False, True), repeat=len(CAPS)):
        ops = _stub(**dict(zip(CAPS, caps)))
        for (q_act, inited, exact, chan), gl, (n_sys, voxels), att_ok, planes_ok in itertools.product(
                flags, (False, True), sizes, (False, True), (False, True)):
            layer = SimpleNamespace(q_act=q_act, _act_inited=inited, lwq_exact_int=exact, channel_wise=chan, qlvl_act=4,
                                    qlvl_w=4)
            want = frozen_specification(ops, geom, layer, True, 32, n_sys, voxels, gl, att_ok, planes_ok)
            p0 = Q.layer_paths(ops, geom, 4, 4, True, 32, n_sys, voxels, q_act=q_act, act_inited=inited, exact_int=exact,
                               channel_wise=chan, gram_loss_enabled=gl, gram_loss_max_n=MAX_N,
                               gram_loss_i8_max_n=I8_MAX_N)
            p1 = p0.after(att_classes_ok=att_ok)
            p2 = p1.after(planes_ok=planes_ok)
            got = _effects(p2)
            gram_call = ("gram_i8(unweighted)" if p1.losses else "gram_i8") if p1.gram_i8 else "gram"
            if want["loss_gram"] is not None and len(want["loss_gram"]) == 4:
                want["loss_gram"] = "four"
            if want["want_idx"] is None:          # no scale is fitted here: the question is never put; the paths say no
                want["want_idx"] = False
            assert got == {k: v for k, v in want.items() if k != "gram_call"} and gram_call == want["gram_call"], \
                (dict(zip(CAPS, caps)), q_act, inited, exact, chan, gl, n_sys, voxels, att_ok, planes_ok, p0, p2, want)
            assert p0.after() == p0 and p2 == p0.after(att_classes_ok=att_ok, planes_ok=planes_ok)
            n_cases += 1
    assert n_cases == 2 ** 7 * 16 * 2 * 10 * 4


def _paths(caps, c1, c2, k, voxels, levels=(4, 4), q_act=True, inited=False, chan=False, exact=True, gl=True):
    import efficientq_amd.qconv as Q
    return Q.layer_paths(_stub(**caps), object(), levels[0], levels[1], True, c2, k ** 3 * c1 + 1, voxels, q_act=q_act,
                         act_inited=inited, exact_int=exact, channel_wise=chan, gram_loss_enabled=gl,
                         gram_loss_max_n=MAX_N, gram_loss_i8_max_n=I8_MAX_N)


def _row(conv, gram_i8, losses, want_idx, fwd_i8):
    """An expected LayerPaths, field by field."""
    import efficientq_amd.qconv as Q
    return Q.LayerPaths(conv=conv, gram_i8=gram_i8, losses=losses, want_idx=want_idx, fwd_i8=fwd_i8)


# the capability answers of the library for the layer class of each row (effq_*_supported)
WIDE32 = dict(ALL, conv_i8s_supported=False, gram_f64_supported=False)                 # 32 -> 32 3^3: K = 864 is not short
FIRST = dict(conv_i8s_supported=True, gram_loss=True, gram_f64_supported=True)         # c1 = 4: no i8 tiles, no i8 Gram
SHORT = dict(ALL, conv_i8_supported=False, conv_i8_out_supported=False, gram_f64_supported=False)   # 1^3
WIDE = dict(ALL, conv_i8s_supported=False, conv_i8_out_supported=False, gram_f64_supported=False)   # 256 / 512 channels

NAMED_ROWS = [
    ("32->32 3^3 at 4/4, voxels below 8 n: integer conv loss", lambda: _paths(WIDE32, 32, 32, 3, 8 * 865 - 1),
     lambda: _row("i8", True, None, True, True), 1),
    ("32->32 3^3 at 4/4, voxels from 8 n: losses from the fp64 Gram system", lambda: _paths(WIDE32, 32, 32, 3, 8 * 865),
     lambda: _row("i8", True, "gram_f64", True, True), 1),
    ("the same with EFFQ_GRAM_LOSS off", lambda: _paths(WIDE32, 32, 32, 3, 8 * 865, gl=False),
     lambda: _row("i8", True, None, True, True), 1),
    ("first conv 4->32 3^3, full-precision input, 256 levels", lambda: _paths(FIRST, 4, 32, 3, 10 ** 6, (-1, 256), q_act=False),
     lambda: _row(None, False, "gram_f64_fp_input", False, False), 0),
    ("the same below 8 n voxels", lambda: _paths(FIRST, 4, 32, 3, 8 * 109 - 1, (-1, 256), q_act=False),
     lambda: _row(None, False, None, False, False), 0),
    ("64->32 1^3: short K, few voxels", lambda: _paths(SHORT, 64, 32, 1, 8 * 65 - 1), lambda: _row("i8s", True, None, True, False), 2),
    ("256->256 3^3 (n = 6913): i8 quadratic form", lambda: _paths(WIDE, 256, 256, 3, 16 * 8 ** 3),
     lambda: _row("i8", True, "gram_i8", True, False), 1),
    ("512->512 3^3 (n = 13825): above GRAM_LOSS_I8_MAX_N, integer conv loss", lambda: _paths(WIDE, 512, 512, 3, 16 * 4 ** 3),
     lambda: _row("i8", True, None, True, False), 1),
    ("32->32 in channel mode: integer Gram system and fp64 Gram losses stay", lambda: _paths(WIDE32, 32, 32, 3, 8 * 865, chan=True),
     lambda: _row(None, True, "gram_f64", True, False), 0),
    ("256->256 in channel mode: no i8 quadratic form", lambda: _paths(WIDE, 256, 256, 3, 16 * 8 ** 3, chan=True),
     lambda: _row(None, True, None, True, False), 0),
    ("32->32 with the activation scale already initialised", lambda: _paths(WIDE32, 32, 32, 3, 8 * 865, inited=True),
     lambda: _row(None, False, None, False, False), 0),
    ("32->32 with lwq_exact_int off", lambda: _paths(WIDE32, 32, 32, 3, 8 * 865, exact=False),
     lambda: _row(None, False, None, False, False), 0),
]


@pytest.mark.parametrize("name,got,want,loss_kind", NAMED_ROWS, ids=[r[0] for r in NAMED_ROWS])
def test_named_layer_classes(name, got, want, loss_kind):
    assert got() == want() and got().loss_kind == loss_kind


def test_facts_known_after_a_call():
    """att_classes() without classes: fp32 Gram system, no losses from it, level ids for the integer conv only, no i8
    forward without level ids.  gram_loss_i8_planes() without planes: only the losses fall back to the conv family."""
    wide32 = _paths(WIDE32, 32, 32, 3, 8 * 865)
    assert wide32.after(att_classes_ok=False) == _row("i8", False, None, True, True)
    chan = _paths(WIDE32, 32, 32, 3, 8 * 865, chan=True)
    assert chan.after(att_classes_ok=False) == _row(None, False, None, False, False)
    no_conv = _paths(dict(WIDE32, conv_i8_supported=False), 32, 32, 3, 8 * 865)
    assert no_conv == _row(None, True, "gram_f64", True, True)
    assert no_conv.after(att_classes_ok=False) == _row(None, False, None, False, False)
    wide = _paths(WIDE, 256, 256, 3, 16 * 8 ** 3)
    assert wide.after(planes_ok=False) == _row("i8", True, None, True, False)
    assert wide.after(planes_ok=False).loss_kind == 1
    assert wide32.after(planes_ok=False) == wide32                 # no planes were asked for


# ---- the sequence of calls one layer's ptq issues ------------------------------------------------------------------

class Recorder:
    """Stands in front of an ops object: forwards everything, and lists each method CALLED, with the arguments that show
    the path (admm_run: loss_kind and which optional keywords were passed; quant_dequant_f64path: want_idx; gram_i8:
    unweighted).  The capability questions (*_supported) answer from shapes alone and enqueue nothing: they are
    forwarded and not listed.  A missing attribute stays missing, so presence tests see the object behind."""

    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        attr = getattr(self._ops, name)
        if not callable(attr) or name.endswith("_supported"):
            return attr

        def call(*a, **kw):
            self.calls.append(self._entry(name, kw))
            return attr(*a, **kw)
        return call

    @staticmethod
    def _entry(name, kw):
        if name == "admm_run":
            opt = ["loss_kind=%d" % kw["loss_kind"]] + (["loss_gram=%d" % len(kw["loss_gram"])] if "loss_gram" in kw else [])
            return "admm_run(" + ", ".join(opt + [k for k in ("channel_wise", "residuals") if k in kw]) + ")"
        if name == "quant_dequant_f64path":
            return f"quant_dequant_f64path(want_idx={bool(kw.get('want_idx', False))})"
        if name == "gram_i8" and kw.get("unweighted"):
            return "gram_i8(unweighted)"
        return name


def record(monkeypatch, ops):
    """Install a Recorder around `ops` at qconv.get_ops and count the tensors ptq hands to its SumReducer."""
    import efficientq_amd.qconv as Q
    rec = Recorder(ops)
    rec.reduced = 0

    class CountingReducer(Q.SumReducer):
        def __call__(self, t):
            rec.reduced += 1
            return super().__call__(t)
    monkeypatch.setattr(Q, "get_ops", lambda device: rec)
    monkeypatch.setattr(Q, "SumReducer", CountingReducer)
    return rec


def make_layer(c1, c2, k, N, S, *, levels=(4, 4), q_act=True, mask=False, seed=11, **kwQ):
    """A seeded layer with its FP target (and an attention mask of three distinct weights): (conv, x)."""
    from efficientq_amd.qconv import EfficientQConvHIP
    gen = torch.Generator().manual_seed(seed)
    conv = EfficientQConvHIP(c1, c2, k, 1, k // 2, 1, 1, True, q_weight=True, qlvl=levels[1], q_act=q_act,
                             qlvl_act=levels[0], **kwQ)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * 0.1)
        conv.bias.copy_(torch.randn(c2, generator=gen) * 0.1)
    x_fp = torch.relu(torch.randn(N, c1, S, S, S, generator=gen))
    conv.output_fp = torch.nn.functional.conv3d(x_fp, conv.weight.data, conv.bias.data, 1, k // 2)
    conv.name, conv.layer_loss = "layer", []
    if mask:
        m = torch.randint(0, 3, (N, S, S, S), generator=gen).float() * 0.5 + 0.5
        conv.mask_pyramid = [torch.ones(N, S // 2, S // 2, S // 2), m]
    return conv, torch.relu(x_fp + 0.05 * torch.randn(x_fp.shape, generator=gen))


STATS = ["moments", "moments"]
TAIL = ["admm_select_best", "conv_step", "admm_read"]
CPU_SEQUENCES = {   # recorded on the commit before the choice of paths became a function (8d13108)
    "plain": (STATS + ["fit_scale", "quant_dequant_f64path(want_idx=False)", "gram", "admm_run(loss_kind=0)"] + TAIL, 2),
    "mask": (STATS + ["moments", "fit_scale", "quant_dequant_f64path(want_idx=False)", "gram", "admm_run(loss_kind=0)"]
             + TAIL, 2),
    "verbose": (STATS + ["fit_scale", "quant_dequant_f64path(want_idx=False)", "gram",
                         "admm_run(loss_kind=0, residuals)"] + TAIL, 2),
}


@pytest.mark.parametrize("case", sorted(CPU_SEQUENCES))
def test_call_sequence_on_the_oracle_backend(monkeypatch, capsys, case):
    """One 4 -> 4 3^3 layer through ptq on the CPU stand-in: the ops methods called, in order, and the number of tensors
    handed to the SumReducer, equal the literals recorded before the refactor.  (12 ADMM iterations: the sequence does
    not depend on their number, and the verbose case still prints two progress lines.)"""
    rec = record(monkeypatch, cpu_backend.OracleOps())
    conv, x = make_layer(4, 4, 3, 1, 6, mask=case == "mask", lwq_verbose=case == "verbose")
    conv.lwq_iter = 12
    conv.set_quantizing()
    with torch.no_grad():
        conv(x)
    out = capsys.readouterr().out
    assert (rec.calls, rec.reduced) == CPU_SEQUENCES[case]
    assert out.count("ADMM iter") == (2 if case == "verbose" else 0)
    assert ("Calibrating layer" in out) == (case == "verbose")
