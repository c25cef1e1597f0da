"""--qconv gptq beside --qconv effq: seconds per calibration and the summed layer_loss on the benchmark's BraTS
configuration (alternating the two in one process; --variants adds gptq with 1 / 2 / 4 refinement passes, with
activation ordering and with R rounds of scale refit and K passes, --channel_wise runs them with one scale per row), and
effq_gptq_chol / effq_gptq_sweep / a pass of effq_gptq_refine / effq_gptq_rescale alone at a few system sizes.

    python scripts/prof_gptq.py calib [--vols 16] [--size 128] [--levels 4] [--steps 3] [--only effq|gptq] [--variants]
                                       [--channel_wise]
    python scripts/prof_gptq.py kernels [n ...]
One JSON line per result."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

PEAK_F64_MFMA_TFLOPS = 78.6       # MI355X fp64 matrix peak (vendor)
PEAK_HBM_GBS = 8000.0             # MI355X HBM3E bandwidth (vendor)
DEV = "cuda:0"


def calib(a):
    from efficientq_amd import calibrate as K, config as Cf, synth
    vols = synth.calib_batch("brats", range(a.vols), a.size).to(DEV)
    nets = {}
    # name: (qconv, passes, order, rounds of scale refit)
    variants = {"effq": ("effq", 0, "natural", 0), "gptq": ("gptq", 0, "natural", 0)}
    if a.variants:
        variants.update({"gptq+r1": ("gptq", 1, "natural", 0), "gptq+r2": ("gptq", 2, "natural", 0),
                         "gptq+r4": ("gptq", 4, "natural", 0), "gptq+act": ("gptq", 0, "act", 0),
                         "gptq+act+r2": ("gptq", 2, "act", 0), "gptq+s1": ("gptq", 0, "natural", 1),
                         "gptq+s1r2": ("gptq", 2, "natural", 1), "gptq+s2r2": ("gptq", 2, "natural", 2)})
    for name in ([a.only] if a.only else variants):
        qconv, passes, order, rounds = variants[name]
        args = Cf.make_args(dict(Cf.BRATS_NET, qconv=qconv), a.levels, a.levels, gptq_refine=passes, gptq_order=order,
                            gptq_rescale=rounds, lwq_channel_wise=a.channel_wise)
        QConv, _, kwQ = Cf.get_conv_class(args)
        model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
        synth.randomise_network(model, 0)
        model.eval()
        K.search_fold_and_remove_bn(model)
        model.to(DEV)
        K.set_name(model)
        nets[name] = (args, model, {k: v.clone() for k, v in model.state_dict().items()})

    def step(name):
        args, model, pristine = nets[name]
        model.load_state_dict(pristine, strict=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = K.calibrate_model(model, vols, "brats", args.init_stride)
        torch.cuda.synchronize()
        return time.perf_counter() - t, sum(float(l.split(":")[1]) for l in res["layer_loss"])

    for name in nets:
        step(name)                                     # warm-up: code objects, workspaces
    times, loss = {name: [] for name in nets}, {}
    for _ in range(a.steps):
        for name in nets:                              # alternating: both see the same state of the machine
            dt, loss[name] = step(name)
            times[name].append(round(dt, 4))
    for name in nets:
        t = sorted(times[name])
        print(json.dumps(dict(metric="calibration", qconv=name, channel_wise=a.channel_wise, vols=a.vols, size=a.size, levels=a.levels,
                              layer_loss_sum=loss[name], seconds=times[name], median_s=t[len(t) // 2])), flush=True)


def kernels(a):
    from efficientq_amd import ops_gptq as OG
    from efficientq_amd.hip_ops import get_ops
    ops = get_ops(DEV)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for n in a.n or (865, 1729, 6913):
        g = torch.Generator().manual_seed(n)
        X = torch.randint(-3, 4, (2 * n, n), generator=g).float().to(DEV)
        A0 = (2 * X.T @ X).contiguous()
        del X
        reps = 10 if n < 4000 else 3
        ms = timed(lambda: OG.gptq_chol(ops, A0, 8.0), reps)
        P = OG.gptq_chol(ops, A0, 8.0, read_flag=True)
        flop = n ** 3 / 3.0
        print(json.dumps(dict(metric="gptq_chol", n=n, ms=round(ms, 3), flop=flop, tflops=round(flop / ms / 1e9, 2),
                              frac_f64_matrix_peak=round(flop / ms / 1e9 / PEAK_F64_MFMA_TFLOPS, 4),
                              launches=OG.gptq_plan(ops, 1, n)["chol_launches"])), flush=True)
        for c2 in (32, 64, 256):
            u = ((torch.rand(c2, n, generator=g) - 0.5)).to(DEV)
            alpha = torch.tensor([0.4], dtype=torch.float64, device=DEV)
            u_w, u_b = u[:, :-1].contiguous(), u[:, -1].contiguous()
            ms = timed(lambda: OG.gptq_sweep(ops, P, n, u_w, u_b, alpha, 4), reps)
            flop = 1.0 * c2 * n * n
            print(json.dumps(dict(metric="gptq_sweep", n=n, c2=c2, ms=round(ms, 3), flop=flop,
                                  tflops=round(flop / ms / 1e9, 3),
                                  frac_f64_matrix_peak=round(flop / ms / 1e9 / PEAK_F64_MFMA_TFLOPS, 5),
                                  launches=OG.gptq_plan(ops, c2, n)["sweep_launches"])), flush=True)
            # a pass alone: the difference of 3 passes and 1 pass over the same sweep state (the moves differ, the launches not)
            G, b, ids, _, row_flag = OG.gptq_sweep(ops, P, n, u_w, u_b, alpha, 4, want_ids=True)
            state, flag = (G.clone(), b.clone(), ids.clone()), OG.gptq_flag(P, n)

            def refine(k):
                for t, t0 in zip((G, b, ids), state):
                    t.copy_(t0)
                OG.gptq_refine(ops, A0, 8.0, u_w, u_b, alpha, 4, k, G, b, ids, row_flag, flag)
            ms1, ms3 = timed(lambda: refine(1), reps), timed(lambda: refine(3), reps)
            print(json.dumps(dict(metric="gptq_refine_pass", n=n, c2=c2, ms=round((ms3 - ms1) / 2, 3),
                                  ms_one_pass_call=round(ms1, 3), flop=2.0 * c2 * n * n,
                                  launches_per_pass=(OG.gptq_refine_plan(ops, c2, n, 2)["launches"] -
                                                     OG.gptq_refine_plan(ops, c2, n, 1)["launches"]))), flush=True)
            # the scale refit: half of the (2 c2) x n x n product (the mirrored half is not multiplied), one read of the
            # triangle of A0
            refine(1)
            a_fit, kept = alpha.clone(), torch.zeros(1, dtype=torch.int32, device=DEV)
            err = torch.empty(c2, dtype=torch.float64, device=DEV)
            ms = timed(lambda: OG.gptq_rescale(ops, A0, 8.0, u_w, u_b, a_fit, 4, G, b, ids, row_flag, flag, out=(err, kept)),
                       reps)
            flop, tri = 2.0 * c2 * n * n, 2.0 * n * (n + 1)
            print(json.dumps(dict(metric="gptq_rescale", n=n, c2=c2, ms=round(ms, 3), flop=flop,
                                  tflops=round(flop / ms / 1e9, 3),
                                  frac_f64_matrix_peak=round(flop / ms / 1e9 / PEAK_F64_MFMA_TFLOPS, 5),
                                  triangle_bytes=tri, frac_hbm_peak=round(tri / ms / 1e6 / PEAK_HBM_GBS, 5),
                                  kept=int(kept.item()), **OG.gptq_rescale_plan(ops, c2, n))), flush=True)
        del A0, P


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    c = sub.add_parser("calib")
    c.add_argument("--vols", type=int, default=16)
    c.add_argument("--size", type=int, default=128)
    c.add_argument("--levels", type=int, default=4)
    c.add_argument("--steps", type=int, default=3)
    c.add_argument("--only", choices=["effq", "gptq"], default=None)
    c.add_argument("--variants", action="store_true")
    c.add_argument("--channel_wise", action="store_true")
    k = sub.add_parser("kernels")
    k.add_argument("n", type=int, nargs="*")
    a = ap.parse_args()
    calib(a) if a.mode == "calib" else kernels(a)
