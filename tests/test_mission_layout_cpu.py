"""The layout of the mission layer (no GPU): evaluate.py is the front of window.py (the sliding window), metrics.py (the
host arithmetic) and reports.py (the CSV writers and the printed reports) and keeps the validation loop; nifti's
BackgroundWriter and prep's read_subjects are the one writer and the one read-ahead loop of the missions."""
import ast
import inspect
import os
import re
import threading

import numpy as np
import pytest
import torch

from efficientq_amd import evaluate, metrics, nifti, prep, reports, window
from efficientq_amd.nifti import BackgroundWriter
from tests.test_post_cpu import SpeckNet
from tests.test_thr_sweep_cpu import SweepOps

MODULES = (window, metrics, reports, evaluate)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every non-dunder callable that evaluate.py defined before it was split, with str(inspect.signature(...)) and its home
CALLABLES = [
    ('_case_geometry', '(geometry, i)', evaluate),
    ('_last_head', "(out) -> 'torch.Tensor'", window),
    ('_lesion_rows', "(rows, shape) -> 'np.ndarray'", evaluate),
    ('_surface_entries', "(ops, logits, lab, kind, fuse, shape, spacing) -> 'dict'", evaluate),
    ('_surface_rows', "(rows, diag: 'float') -> 'torch.Tensor'", metrics),
    ('_sweep_ints', '(hist)', metrics),
    ('_triple', '(v)', window),
    ('_vs_fp', "(ops, q, f, kind, fuse, shape, spacing, lesions, surface, want_map) -> 'dict'", evaluate),
    ('_write_map', '(path, host, dtype, entry=None)', evaluate),
    ('agreement_means', "(results) -> 'dict'", metrics),
    ('check_flips', "(flips) -> 'tuple'", window),
    ('dice', "(pred_b: 'torch.Tensor', target_b: 'torch.Tensor') -> 'torch.Tensor'", metrics),
    ('fp_vs_quantised_dice', "(model_q, images: 'torch.Tensor', task: 'str', fp_model=None, fp_logits=None, "
                             "patch_size=64, overlap=16)", evaluate),
    ('image_to_patch3d', "(images: 'torch.Tensor', patch_sz, overlap) -> 'List[torch.Tensor]'", window),
    ('label_rule', "(multi: 'bool', multi_label=None, task: 'str' = 'lits') -> 'str'", evaluate),
    ('lesion_size_summary', "(results) -> 'np.ndarray'", metrics),
    ('lesion_totals', "(results) -> 'torch.Tensor'", metrics),
    ('logit_prob', "(logit: 'float') -> 'float'", metrics),
    ('metric_means', "(results) -> 'dict'", metrics),
    ('metrics_from_counts', "(counts: 'torch.Tensor') -> 'dict'", metrics),
    ('mirror_flips', "(axes) -> 'tuple'", window),
    ('patch_to_image3d', "(images: 'torch.Tensor', patch_list: 'Sequence[torch.Tensor]', patch_sz, overlap) -> "
                         "'torch.Tensor'", window),
    ('post_class_lut', "(rule: 'str', C: 'int') -> 'list'", evaluate),
    ('post_means', "(results) -> 'dict'", metrics),
    ('post_refusal', "(rule: 'str') -> 'str'", evaluate),
    ('sliding_window_forward', "(model, images: 'torch.Tensor', patch_size=64, overlap=16) -> 'torch.Tensor'", window),
    ('stitched_window_logits', "(ops, nets, vol: 'torch.Tensor', patch, overlap, window_batch=None, blend='uniform', "
                               "flips=(0,))", window),
    ('surface_means', "(results) -> 'torch.Tensor'", metrics),
    ('surface_metrics', "(counts, sums, shape) -> 'torch.Tensor'", metrics),
    ('surface_metrics_mm', "(counts, sq, sums, shape, spacing) -> 'torch.Tensor'", metrics),
    ('sweep_pooled', '(hists)', metrics),
    ('sweep_results', '(results)', metrics),
    ('sweep_summary', '(hist, edges)', metrics),
    ('validate_seg', "(model, loader, task: 'str', patch_size, overlap, window_batch=None, fuse=None, names=None, "
                     "save_dir=None, label_dtype=<class 'numpy.uint16'>, multi_label=None, lesions=False, surface=False, "
                     "geometry=None, lesion_table=False, fp_model=None, blend='uniform', flips=(0,), post=None, "
                     "post_conn=26, sweep=False, lesion_match=False)", evaluate),
    ('validate_vs_label', "(output: 'torch.Tensor', target: 'torch.Tensor', task: 'str' = 'lits')", metrics),
    ('window_starts', "(size: 'int', patch: 'int', overlap: 'int') -> 'List[int]'", window),
    ('write_agreement_csv', "(path: 'str', results) -> 'None'", reports),
    ('write_lesions_csv', "(path: 'str', results) -> 'None'", reports),
    ('write_metrics_csv', "(path: 'str', results) -> 'None'", reports),
    ('write_metrics_post_csv', "(path: 'str', results) -> 'None'", reports),
    ('write_threshold_csv', "(path: 'str', results) -> 'None'", reports),
    ('write_threshold_curve_csv', "(path: 'str', results) -> 'None'", reports),
]
# and every upper-case constant, with its value
CONSTANTS = [
    ('AGREEMENT_COUNTS', ('both', 'q_only', 'fp_only', 'neither'), metrics),
    ('AGREEMENT_DRIFT', ('logit_rel_mse', 'logit_max', 'prob_mae'), metrics),
    ('BLEND_KINDS', ('uniform', 'gauss'), window),
    ('EPS', 1e-6, metrics),
    ('LESION_COLUMNS', ('totall', 'predl', 'fnl', 'fpl'), metrics),
    ('LESION_SIZE_BINS', ((1, 9), (10, 99), (100, 999), (1000, None)), metrics),
    ('LESION_TABLE_COLUMNS', ('d', 'h', 'w', 'size', 'overlap'), metrics),
    ('METRICS', ('dsc', 'sens', 'spec', 'acc'), metrics),
    ('MIRROR_AXES', 'dhw', window),
    ('SURFACE_COLUMNS', ('hd', 'hd95', 'assd'), metrics),
    ('SURFACE_COLUMNS_MM', ('hd_mm', 'hd95_mm', 'assd_mm'), metrics),
    ('SWEEP_BINS', 4096, metrics),
    ('SWEEP_MID', 2048, metrics),
    ('THRESHOLD_COLUMNS', ('subject', 'class', 'auc', 'dsc', 'best_thr_logit', 'best_thr_prob', 'dsc_best', 'sens_best',
                           'spec_best', 'pos', 'neg'), reports),
    ('THRESHOLD_CURVE_COLUMNS', ('class', 'k', 'thr_logit', 'thr_prob', 'tp', 'fp', 'fn', 'tn', 'dsc', 'sens', 'spec'),
     reports),
    ('WINDOW_BATCH_MAX', 16, window),
]


# ---- the surface -----------------------------------------------------------------------------------------------------------
def test_evaluate_keeps_every_name_with_its_signature_and_its_object():
    assert len(CALLABLES) == 42 and len(CONSTANTS) == 16
    for name, sig, home in CALLABLES:
        fn = getattr(evaluate, name)
        assert callable(fn) and str(inspect.signature(fn)) == sig, name
        assert getattr(home, name) is fn, f"evaluate.{name} is not {home.__name__}.{name}"
    for name, value, home in CONSTANTS:
        assert getattr(evaluate, name) == value, name
        assert getattr(home, name) is getattr(evaluate, name), f"evaluate.{name} is not {home.__name__}.{name}"


def _defined(mod):
    """The names a module's own text defines at its top level: def, class and assignment."""
    names = set()
    for node in ast.parse(inspect.getsource(mod)).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            names.add(node.name)
        elif isinstance(node, (ast.Assign, ast.AnnAssign)):
            targets = node.targets if isinstance(node, ast.Assign) else [node.target]
            names.update(t.id for t in targets if isinstance(t, ast.Name))
    return names


def test_no_name_is_defined_by_two_modules():
    owner = {}
    for mod in MODULES:
        for name in _defined(mod):
            assert name not in owner, f"{name} is defined by {owner[name].__name__} and by {mod.__name__}"
            owner[name] = mod
    for name, _, home in CALLABLES + CONSTANTS:
        if name not in ("_triple", "BLEND_KINDS"):       # these two come from ops_base and ops_window
            assert owner[name] is home, name


def test_a_constant_that_tests_or_scripts_assign_lives_in_evaluate_alone():
    """A test that assigns to evaluate.X must reach every user of X: a copy in another module would not follow it."""
    names = "|".join(name for name, _, _ in CONSTANTS)
    assigned = set()
    for folder in ("tests", "scripts"):
        for fn in sorted(os.listdir(os.path.join(ROOT, folder))):
            if fn.endswith(".py") and fn != os.path.basename(__file__):
                with open(os.path.join(ROOT, folder, fn)) as f:
                    text = f.read()
                for m in re.finditer(rf"""setattr\(\s*\w+\s*,\s*["']({names})["']|\b(?:E|evaluate)\.({names})\s*=[^=]""", text):
                    assigned.add(m.group(1) or m.group(2))
    for name in assigned:
        for mod in (window, metrics, reports):
            assert not hasattr(mod, name), f"{mod.__name__}.{name} is a copy that an assignment to evaluate.{name} misses"


# ---- the writer --------------------------------------------------------------------------------------------------------------
def _live(prefix):
    return [t.name for t in threading.enumerate() if t.name.startswith(prefix)]


def test_writer_with_a_bound_waits_for_the_oldest_job():
    gates, done, seen = [threading.Event() for _ in range(3)], [], []

    def job(i):
        assert gates[i].wait(10)
        done.append(i)
    with BackgroundWriter("effq-test-bound", 2) as w:
        w.submit(job, 0)
        w.submit(job, 1)

        def third():
            w.submit(job, 2)
            seen.append(list(done))
        t = threading.Thread(target=third)
        t.start()
        t.join(0.05)
        assert t.is_alive() and seen == []          # two jobs pending: the third submit has not returned
        gates[0].set()
        t.join(10)
        assert not t.is_alive() and seen == [[0]]   # it returned once the first job had finished, and no later
        gates[1].set()
        gates[2].set()
    assert done == [0, 1, 2] and _live("effq-test-bound") == []


def test_writer_reraises_a_failed_job_on_exit_after_the_others_have_run():
    ran = []

    def fail():
        raise OSError("disk full")
    with pytest.raises(OSError, match="disk full"):
        with BackgroundWriter("effq-test-fail") as w:
            w.submit(ran.append, 1)
            w.submit(fail)
            w.submit(ran.append, 3)
    assert ran == [1, 3] and _live("effq-test-fail") == []


def test_writer_joins_its_thread_when_the_body_raises():
    ran, gate = [], threading.Event()

    def job():
        assert gate.wait(10)
        ran.append("written")
    with pytest.raises(KeyError, match="body"):
        with BackgroundWriter("effq-test-body") as w:
            w.submit(job)
            assert _live("effq-test-body")
            gate.set()
            raise KeyError("body")
    assert ran == ["written"] and _live("effq-test-body") == []


def test_writer_runs_and_returns_in_submission_order():
    ran = []

    def job(i):
        ran.append(i)
        return i * i
    with BackgroundWriter("effq-test-order", 3) as w:
        jobs = [w.submit(job, i) for i in range(8)]
    assert ran == list(range(8)) and [j.result() for j in jobs] == [i * i for i in range(8)]


# ---- the reader ----------------------------------------------------------------------------------------------------------------
class _Plan:
    def __init__(self, sn):
        self.subject, self.entry = sn, {"subject": sn}


@pytest.mark.parametrize("prefix", ["effq-prep-read", "effq-predict-read"])
def test_reader_reads_ahead_names_a_failed_read_and_leaves_no_thread(monkeypatch, prefix):
    started = {sn: threading.Event() for sn in "abc"}
    order = []

    def load(entry, mods):
        sn = entry["subject"]
        order.append(sn)
        started[sn].set()
        assert threading.current_thread().name.startswith(prefix) and mods == ("ct",)
        return ({"ct": sn.upper()}, None)
    monkeypatch.setattr(prep, "_load", load)
    plans = [_Plan(sn) for sn in "abc"]
    gen = prep.read_subjects(plans, ("ct",), prefix)
    first = next(gen)
    assert first == (plans[0], {"ct": "A"}, None)
    assert started["b"].wait(10) and not started["c"].is_set()      # b is being read while a is the caller's
    assert [got[0].subject for got in gen] == ["b", "c"] and order == ["a", "b", "c"] and _live(prefix) == []
    # a failed read arrives as the PrepError of its subject, when that subject is asked for
    monkeypatch.setattr(prep, "_load", lambda entry, mods: ValueError("boom") if entry["subject"] == "b" else ({}, None))
    gen = prep.read_subjects(plans, ("ct",), prefix)
    assert next(gen)[0].subject == "a"
    with pytest.raises(prep.PrepError, match="subject b: boom"):
        next(gen)
    assert _live(prefix) == []
    # closed after the first subject: the pending read is dropped or finished, and the thread is gone
    monkeypatch.setattr(prep, "_load", load)
    gen = prep.read_subjects(plans, ("ct",), prefix)
    assert next(gen)[0].subject == "a"
    gen.close()
    assert _live(prefix) == [] and "c" not in order[3:]


# ---- the batches ---------------------------------------------------------------------------------------------------------------
class BatchOps(SweepOps):
    """SweepOps with lesion counts that are a plain function of the case's decisions and label (C x 4 int64)."""

    def seg_lesions(self, logits, label, task, fuse=None):
        pred = logits.argmax(0)
        return torch.stack([torch.stack([(label == c).sum(), (pred == c).sum(), ((label == c) & (pred != c)).sum(),
                                         ((label != c) & (pred == c)).sum()]) for c in range(logits.shape[0])])


def _same(a, b, where):
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and torch.equal(a, b), where
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b), where
    else:
        assert a == b, where


def test_one_batch_of_two_cases_gives_what_two_batches_of_one_give(monkeypatch, tmp_path):
    from efficientq_amd import hip_ops
    ops = BatchOps()
    monkeypatch.setattr(hip_ops, "get_ops", lambda dev: ops)
    g = torch.Generator().manual_seed(11)
    shape = (12, 10, 9)             # patch 8, overlap 4: two windows along every axis
    imgs, labs = torch.randn(2, 1, *shape, generator=g), torch.randint(0, 3, (2,) + shape, generator=g)
    kw = dict(task="lits", patch_size=(8, 8, 8), overlap=(4, 4, 4), window_batch=4, names=["a", "b"], lesions=True,
              post=[((1, 2), "largest", 0, 0), ((2,), "min", 3, 1)], post_conn=6, sweep=True)
    assert ops.window_grid(shape, (8, 8, 8), (4, 4, 4)) == (2, 2, 2)
    one = evaluate.validate_seg(SpeckNet(), [(imgs, labs)], save_dir=str(tmp_path / "one"), **kw)
    two = evaluate.validate_seg(SpeckNet(), [(imgs[:1], labs[:1]), (imgs[1:], labs[1:])], save_dir=str(tmp_path / "two"),
                                **kw)
    assert len(one) == len(two) == 2 and [r["name"] for r in one] == ["a", "b"]
    assert list(one[0]) == ["name", "counts", "dsc", "sens", "spec", "acc", "sweep", "sweep_edges", "lesions", "post"]
    _same(one, two, "results")
    assert not torch.equal(one[0]["counts"], one[1]["counts"]) and sum(one[0]["post"]["changed"]) > 0
    for sn in ("a", "b"):
        a, b = (nifti.read_nifti(str(tmp_path / d / f"{sn}.nii.gz"))[0] for d in ("one", "two"))
        assert a.shape == shape and a.dtype == np.uint16 and np.array_equal(a, b)
    assert not np.array_equal(nifti.read_nifti(str(tmp_path / "one" / "a.nii.gz"))[0],
                              nifti.read_nifti(str(tmp_path / "one" / "b.nii.gz"))[0])
