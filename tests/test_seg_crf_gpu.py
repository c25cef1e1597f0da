"""effq_seg_crf against the fp64 restatement (tests/seg_crf_ref.py), and predict --crf end to end.

The bar on H after T iterations, eps = 2^-24, Wt = w_a + w_s, N the offsets of the neighbourhood:
  * one message sum_j k_j q_j with sum_j k_j <= Wt and |q_j| <= 1.  The exponent of a pair is M multiply-adds of rounded
    differences times a folded constant, (M + 4) eps relative; through exp2 that is at most (M + 4) eps / e absolute (u e^-u
    <= 1 / e), plus the instruction's 1 ulp: (M + 6) eps.  With the two table entries rounded once and the multiply-add:
    |dk_j| <= w_a g_p (M + 6) eps + 2 eps k_j, summed over the pairs  w_a (M + 6) eps + 2 eps Wt.
  * q_j: the softmax of C exponentials through exp2 and one division, at most (4.2 C + 4.2) eps absolute; 2 sigmoid - 1 at
    most 7 eps: (5 C + 8) eps holds both, times sum k_j <= Wt.
  * N multiply-adds into an accumulator that never exceeds Wt: N eps Wt; the sum with v: eps (max |v| + Wt).
  b1 = eps (w_a (M + 6) + 2 Wt + Wt (5 C + 8) + N Wt + max |v| + Wt).
  * An error d of H enters the next message through q with the Lipschitz constant L = Wt / 2 (the infinity norm of the
    softmax Jacobian and of 2 sigmoid' is at most 1 / 2):  bar(T) = b1 (1 + L + ... + L^(T - 1)).
The decisions taken from H, and `changed`, may differ from the restatement's only at voxels whose fp64 margin is below
twice the bar; their share is computed from the restatement alone and must stay under 1 %."""
import csv
import os

import numpy as np
import pytest
import torch

from efficientq_amd import calibrate as K, config as Cf, crf, data as D, evaluate as E, nifti, ops_crf, predict, prep, synth
from efficientq_amd.hip_ops import get_ops
from tests import seg_crf_ref as R
from tests.test_prep_cpu import write_scan

pytestmark = pytest.mark.gpu
DEV, EPS32 = "cuda:0", 2.0 ** -24
TD, TH, TW = ops_crf.TILE
W_A, W_S, THETAS = 4.0, 1.0, (3.0, 0.5, 1.0)
EXCUSED_SHARE_MAX = 0.01


def bar(C, M, n_offsets, iters, vmax):
    wt = W_A + W_S
    b1 = EPS32 * (W_A * (M + 6) + 2 * wt + wt * (5 * C + 8) + n_offsets * wt + vmax + wt)
    return b1 * sum((wt / 2) ** t for t in range(iters))


@pytest.fixture(scope="module")
def ops():
    return get_ops(DEV)


def volume(shape, C, M, poison=False):
    """Seeded normal logits times 4; images: a smooth ramp plus a step edge plus noise of 0.2."""
    g = np.random.default_rng(C * 1000 + M * 100 + sum(shape))
    v = (4.0 * g.standard_normal((C,) + shape)).astype(np.float32)
    d, h, w = np.meshgrid(*[np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1) for n in shape], indexing="ij")
    x = np.stack([(0.5 + 0.1 * m) * (d + h - w) + (h + 0.3 * w > 0.1 * m) + 0.2 * g.standard_normal(shape) for m in range(M)])
    x = x.astype(np.float32)
    if poison:      # a NaN logit, an Inf intensity, and one voxel with both next to the first: neighbours of each kind
        v[1, 2, 3, 3], x[M - 1, 3, 4, 5] = np.nan, np.inf
        v[0, 2, 3, 4], x[0, 2, 3, 4] = -np.inf, np.nan
    return v, x


def check(v, x, spacing, mode, iters, got, changed, thresh=0.0):
    """`got` (fp32 H of the device) and `changed` against the restatement at the bar; returns the excused voxels and the
    restatement's H and count."""
    want, changed_ref, ok = R.crf(v, x, spacing, mode, W_A, W_S, *THETAS, iters, thresh)
    n = len(R.offsets(R.radii(spacing, THETAS[0], THETAS[2])))
    b = bar(v.shape[0], x.shape[0], n, iters, float(np.abs(v[:, ok]).max()))
    assert np.array_equal(got.view(np.uint32)[:, ~ok], v.view(np.uint32)[:, ~ok])        # bit for bit
    err = float(np.abs(got[:, ok].astype(np.float64) - want[:, ok]).max())
    unsure = ok & (R.margin(want, mode, thresh) < 2 * b)
    print(f"{v.shape} M {x.shape[0]} {mode} T {iters} spacing {spacing}: error {err:.3g} of the bar {b:.3g} "
          f"({err / b:.3g}), {int(unsure.sum())} of {int(ok.sum())} voxels excused, changed {changed} / {changed_ref}")
    assert unsure.sum() <= EXCUSED_SHARE_MAX * ok.sum()                                   # from the restatement alone
    assert err <= b
    sure = ok & ~unsure
    assert np.array_equal(R.decide(got, mode, thresh)[sure], R.decide(want, mode, thresh)[sure])
    assert abs(changed - changed_ref) <= int(unsure.sum())
    return unsure, want, changed_ref


CASES = [((2, 3, 2), 2, 1, "softmax", (1, 1, 1), 1, False),
         ((TD + 1, TH + 1, TW + 1), 3, 4, "softmax", (1, 1, 1), 1, False),
         ((TD + 1, TH + 1, TW + 1), 3, 4, "softmax", (1, 1, 1), 5, False),
         ((TD + 1, TH + 1, TW + 1), 3, 4, "sigmoid", (1, 1, 1), 1, False),
         ((TD + 1, TH + 1, TW + 1), 3, 4, "sigmoid", (1, 1, 1), 5, False),
         ((2 * TD + 3, TH - 1, TW - 1), 8, 4, "softmax", (1, 1, 1), 5, False),
         ((9, 10, TW + 3), 3, 2, "softmax", (2.5, 0.8, 0.8), 5, False),
         ((5, TH + 1, TW + 2), 2, 1, "softmax", (7, 1, 1), 5, False),
         ((5, TH + 1, TW + 2), 3, 4, "softmax", (1, 1, 2.5), 5, False),          # radii 3 3 2: the rolled row of pairs
         ((TD + 1, TH + 2, 2 * TW + 1), 3, 2, "sigmoid", (0.8, 2.5, 7), 5, False),       # radii 3 2 0: no halo along W
         ((6, 7, 8), 3, 2, "softmax", (1, 1, 1), 1, True)]


@pytest.mark.parametrize("shape, C, M, mode, spacing, iters, poison", CASES)
def test_the_kernel_against_the_restatement(ops, shape, C, M, mode, spacing, iters, poison):
    v, x = volume(shape, C, M, poison)
    run = lambda: ops_crf.seg_crf(ops, torch.from_numpy(v).to(DEV), torch.from_numpy(x).to(DEV), spacing, mode, W_A, W_S,
                                  *THETAS, iters)
    got, changed = run()
    check(v, x, spacing, mode, iters, got.cpu().numpy(), changed)
    again, changed_again = run()
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and changed == changed_again


def test_predict_with_crf_end_to_end(ops, tmp_path):
    root, out = str(tmp_path), str(tmp_path / "seg")
    os.makedirs(os.path.join(root, "src"))
    g = np.random.default_rng(7)
    scan = np.zeros((36, 38, 34), dtype=np.int16)
    scan[2:-2, 2:-2, 1:-1] = g.integers(-400, 500, size=(32, 34, 32))
    write_scan(os.path.join(root, "src", "a.nii.gz"), scan, affine=np.diag([2.0, 1.0, 1.0, 1.0]))
    lst = os.path.join(root, "cases.csv")
    with open(lst, "w") as f:
        f.write("subject,ct\na,src/a.nii.gz\n")
    args = Cf.make_args(dict(Cf.TINY_NET, qconv="conv"), 4, 4, src_list=lst, out_dir=out, patch_size="32,32,32",
                        prep_mask="nonzero", merge_type=None, crf=True)
    model = Cf.get_model_cube(args)[0]["model"]
    synth.randomise_network(model, 0)
    model.eval()
    K.search_fold_and_remove_bn(model)
    model.to(DEV)
    K.set_fp(model)
    rows = predict.run(args, model=model, window_batch=1)

    patch, overlap = (32, 32, 32), (16, 16, 16)
    entry = prep.read_src_list(lst, "lits")[0]
    plan = prep._Plan(entry, ("ct",), None, patch)
    assert tuple(plan.grid_spacing) == (2.0, 1.0, 1.0)
    imgs = {"ct": nifti.read_image(entry["images"]["ct"])[0]}
    y, _, _, pmin, pmax, _, _, _ = prep.process_subject(
        ops, plan, imgs, None, ("ct",), prep.PrepOptions("nonzero", (-200.0, 250.0), None, patch, False))
    vol = torch.from_numpy(y)[None].to(DEV)
    outs, _, _ = E.stitched_window_logits(ops, [model], vol, patch, overlap, 1)
    v, x = outs[0][0].cpu().numpy(), y
    got, changed = ops_crf.seg_crf(ops, outs[0][0].contiguous(), vol[0], plan.grid_spacing, "softmax", *crf.DEFAULTS)
    assert (W_A, W_S) + THETAS + (5,) == crf.DEFAULTS
    unsure, want_h, changed_ref = check(v, x, (2.0, 1.0, 1.0), "softmax", 5, got.cpu().numpy(), changed)
    want_h = torch.from_numpy(want_h.astype(np.float32)).to(DEV)
    where = (pmin, plan.grid_shape, plan.factors, plan.oriented_shape)                   # as predict._segment decides it
    want = predict._on_scan_grid(ops, plan, ops.seg_labels_source(want_h, *where, "argmax", args.merge_type)).cpu().numpy()
    box = torch.from_numpy(D.restore_crop(unsure.astype(np.uint8), pmin, pmax, plan.oriented_shape)).to(DEV)
    sure = ~predict._on_scan_grid(ops, plan, box).cpu().numpy().astype(bool)
    written, _ = nifti.read_nifti(os.path.join(out, "a.nii.gz"))
    assert written.shape == scan.shape and np.array_equal(written[sure], want[sure]) and len(np.unique(written)) > 1
    with open(os.path.join(out, predict.PREDICT_CSV)) as f:
        header, row = list(csv.reader(f))
    assert header[-2:] == ["crf", "crf_changed"] == predict.CSV_CRF_COLUMNS and rows[0]["crf"] == row[-2] == "4 1 3 0.5 1 5"
    assert int(row[-1]) == changed and abs(changed - changed_ref) <= int(unsure.sum())
