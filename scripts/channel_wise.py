"""Channel mode (lwq_channel_wise) against per-tensor mode on the GPU.

    python scripts/channel_wise.py kernels            # the weight-scale fixed point alone, per channel vs per tensor
    python scripts/channel_wise.py calib [reps] [vols] [size]   # whole BraTS calibration, both modes alternating

`kernels` times, with HIP events, the per-channel kernel (effq_fixed_point_channels) and the per-tensor kernel the ADMM
loop uses at the same size (effq_fixed_point_small up to 32768 weights, the bucketed one up to 2^19, the cooperative one
above) on the weights of the BraTS layers (4 and 16 levels) and of the first conv (256 levels).  The values are a
weight-like tensor w* + dual with output-channel norms spread by 2^(c mod 4), as BN folding leaves them.  Run it under
`rocprofv3 --kernel-trace --stats -- python ...` for the per-kernel figures.

`calib` runs BASELINE.json configs[1] (16 synthetic volumes 4 x 128^3, 4 levels) `reps` times in each mode, alternating,
in one process, and prints seconds per calibration, the loss path every layer took and the per-layer layer_loss."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

DEV = "cuda:0"


def kernels():
    from efficientq_amd.hip_ops import get_ops
    ops = get_ops(DEV)
    gen = torch.Generator().manual_seed(0)
    # (c2, nwrow, levels): BraTS 3^3 layers 32 / 64 / 128 / 256 channels (c1 = c2, c2 / 2 at the up path), first conv
    cases = [(32, 864, 4), (64, 1728, 4), (128, 3456, 4), (256, 6912, 4), (128, 6912, 4), (64, 3456, 4), (32, 1728, 4),
             (32, 864, 16), (64, 1728, 16), (128, 3456, 16), (256, 6912, 16), (32, 108, 256)]
    for c2, nwrow, L in cases:
        n = c2 * nwrow
        s = torch.tensor([2.0 ** (c % 4) for c in range(c2)]).unsqueeze(1)
        w = (torch.randn(c2, nwrow, generator=gen) * 0.05 * s).to(DEV)
        du = (torch.randn(c2, nwrow, generator=gen) * 0.005 * s).to(DEV)
        v = torch.empty_like(w)
        alpha = torch.empty(c2, dtype=torch.float64, device=DEV)
        iters = torch.empty(c2, dtype=torch.int32, device=DEV)
        st = ops.new_fp_state()
        if n <= ops.lib.effq_fp_small_max():
            per_tensor = ("small", lambda: ops.weight_fixed_point(w, du, v, L, st))
        elif n <= (1 << 19) and L <= 16:
            per_tensor = ("bucket", lambda: ops.fixed_point_bucket(w, du, v, L, st))
        else:
            per_tensor = ("coop", lambda: ops.weight_fixed_point(w, du, v, L, st))
        res = {}
        for name, fn in (("channels", lambda: ops.fixed_point_channels(w, du, v, L, alpha, iters)), per_tensor):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name] = e0.elapsed_time(e1) / 50 * 1e3
        it = iters.cpu()
        print(f"c2={c2:4d} nwrow={nwrow:5d} weights={n:8d} L={L:3d}  per channel {res['channels']:7.1f} us "
              f"(row iterations max {int(it.max())} mean {float(it.float().mean()):.1f})  per tensor [{per_tensor[0]}] "
              f"{res[per_tensor[0]]:7.1f} us ({ops.read_fp_state(st)[1]} iterations)", flush=True)


def calib(reps=2, nvol=16, size=128):
    from efficientq_amd import calibrate as K, config as Cf, synth
    from efficientq_amd.qconv import EfficientQConvHIP
    models = {}
    for cw in (False, True):
        args = Cf.make_args(Cf.BRATS_NET, 4, 4, lwq_channel_wise=cw)
        QConv, _, kwQ = Cf.get_conv_class(args)
        model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
        synth.randomise_network(model, 0)
        model.eval()
        K.search_fold_and_remove_bn(model)
        model.to(DEV)
        K.set_name(model)
        models[cw] = (args, model, {k: v.clone() for k, v in model.state_dict().items()})
    vols = synth.calib_batch("brats", range(nvol), size).to(DEV)
    times = {False: [], True: []}
    last = {}
    for rep in range(reps + 1):                     # pass 0 of each mode: warm-up
        for cw in (False, True):
            args, model, pristine = models[cw]
            model.load_state_dict(pristine)
            torch.cuda.synchronize()
            t0 = time.time()
            res = K.calibrate_model(model, vols, "brats", args.init_stride)
            torch.cuda.synchronize()
            dt = time.time() - t0
            if rep > 0:
                times[cw].append(dt)
            print(f"pass {rep} {'channel' if cw else 'tensor '}: {dt:.3f} s", flush=True)
            last[cw] = (res["layer_loss"], [(m.name, dict(m.last_trace)) for m in model.modules()
                                            if isinstance(m, EfficientQConvHIP) and m.last_trace is not None])
    for cw in (False, True):
        ts = times[cw]
        print(f"{'channel' if cw else 'tensor '} mode: {sum(ts) / len(ts):.3f} s per calibration "
              f"(min {min(ts):.3f}, {len(ts)} runs)")
    print(f"{'layer':45s} {'loss path (tensor -> channel)':34s} {'layer_loss tensor':>18s} {'channel':>12s} {'ratio':>7s}")

    def kind(tr):            # gram: loss kinds 4 / 5 (Gram system), int-conv: 1 / 2, f32-conv: 0
        if tr["paths"]["losses"]:
            return "gram"
        return "int-conv" if tr["paths"]["conv"] else "f32-conv"
    tot = {False: 0.0, True: 0.0}
    for (name, tr_t), (_, tr_c) in zip(last[False][1], last[True][1]):
        lt, lc = tr_t["layer_loss"], tr_c["layer_loss"]
        tot[False] += lt
        tot[True] += lc
        print(f"{name:45s} {kind(tr_t) + ' -> ' + kind(tr_c):34s} {lt:18.6g} {lc:12.6g} {lc / lt:7.3f}  "
              f"admm loop {tr_t['admm_loop_s'] * 1e3:7.1f} -> {tr_c['admm_loop_s'] * 1e3:7.1f} ms")
    print(f"{'sum':45s} {'':34s} {tot[False]:18.6g} {tot[True]:12.6g} {tot[True] / tot[False]:7.3f}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if mode == "kernels":
        kernels()
    else:
        calib(*(int(a) for a in sys.argv[2:]))
