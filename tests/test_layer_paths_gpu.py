"""Which kernels the layer classes of the product take on a real MI355X (-m gpu): last_trace["paths"] and the sequence of
ops calls of EfficientQConvHIP.ptq, against literals recorded on the commit before the choice of paths became a function
(8d13108), on the smallest shapes that reach each path."""
import pytest
import torch

from tests.test_layer_paths_cpu import make_layer, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

STATS = ["moments", "moments"]
QUANT = ["fit_scale", "quant_dequant_f64path(want_idx=True)"]
READ = ["admm_select_best", "conv_step", "admm_read", "release_retired"]
READ_I8 = ["admm_select_best", "conv_forward_i8", "admm_read", "release_retired"]

# name: (make_layer arguments, attributes set on the layer, paths, calls)
LAYERS = {
    # the kernel of the i8 forward stores whole 8 x 4 x 8 output tiles (effq_conv_i8_out_supported): S = 8 has them,
    # S = 12 and S = 20 do not and take the integer losses with the fused fp32 forward
    "32->32 3^3 N=2 S=8: integer conv loss, i8 forward": (
        dict(c1=32, c2=32, k=3, N=2, S=8), {},
        dict(conv="i8", gram_i8=True, losses=None, want_idx=True, fwd_i8=True),
        STATS + ["att_classes"] + QUANT + ["gram_i8", "admm_run(loss_kind=1)"] + READ_I8),
    "32->32 3^3 N=2 S=12: integer conv loss": (
        dict(c1=32, c2=32, k=3, N=2, S=12), {},
        dict(conv="i8", gram_i8=True, losses=None, want_idx=True, fwd_i8=False),
        STATS + ["att_classes"] + QUANT + ["gram_i8", "admm_run(loss_kind=1)"] + READ),
    "32->32 3^3 N=2 S=20: losses from the fp64 Gram system": (
        dict(c1=32, c2=32, k=3, N=2, S=20), {},
        dict(conv="i8", gram_i8=True, losses="gram_f64", want_idx=True, fwd_i8=False),
        STATS + ["att_classes"] + QUANT + ["gram_i8(unweighted)", "admm_run(loss_kind=1, loss_gram=3)"] + READ),
    "32->32 3^3 N=2 S=20 with an attention mask": (
        dict(c1=32, c2=32, k=3, N=2, S=20, mask=True), {},
        dict(conv="i8", gram_i8=True, losses="gram_f64", want_idx=True, fwd_i8=False),
        STATS + ["moments", "att_classes"] + QUANT + ["gram_i8(unweighted)", "admm_run(loss_kind=1, loss_gram=3)"] + READ),
    "4->32 3^3 full-precision input: fp64 Gram system of the input": (
        dict(c1=4, c2=32, k=3, N=2, S=12, levels=(-1, 256), q_act=False), {},
        dict(conv=None, gram_i8=False, losses="gram_f64_fp_input", want_idx=False, fwd_i8=False),
        STATS + ["gram", "gram_f64", "admm_run(loss_kind=0, loss_gram=3)"] + READ),
    "64->32 1^3 N=2 S=6: short-K kernel": (
        dict(c1=64, c2=32, k=1, N=2, S=6), {},
        dict(conv="i8s", gram_i8=True, losses=None, want_idx=True, fwd_i8=False),
        STATS + ["att_classes"] + QUANT + ["gram_i8", "admm_run(loss_kind=2)"] + READ),
    # lwq_iter lowered to 8 on this one: the sequence does not depend on it, and 200 iterations of a 6913-row system
    # with its four inverses would take this case out of the few seconds a test may take
    "256->256 3^3 N=1 S=6: i8 quadratic form": (
        dict(c1=256, c2=256, k=3, N=1, S=6), dict(lwq_iter=8),
        dict(conv="i8", gram_i8=True, losses="gram_i8", want_idx=True, fwd_i8=False),
        STATS + ["att_classes"] + QUANT + ["gram_i8(unweighted)", "gram_loss_i8_planes",
                                           "admm_run(loss_kind=1, loss_gram=4)"] + READ),
    "32->32 3^3 N=2 S=20 in channel mode": (
        dict(c1=32, c2=32, k=3, N=2, S=20, lwq_channel_wise=True), {},
        dict(conv=None, gram_i8=True, losses="gram_f64", want_idx=True, fwd_i8=False),
        STATS + ["att_classes"] + QUANT + ["gram_i8(unweighted)", "admm_run(loss_kind=0, loss_gram=3, channel_wise)"]
        + READ),
    "32->32 3^3 N=2 S=12 with _act_inited": (
        dict(c1=32, c2=32, k=3, N=2, S=12), dict(_act_inited=True),
        dict(conv=None, gram_i8=False, losses=None, want_idx=False, fwd_i8=False),
        STATS + ["quant_dequant_f32", "gram", "admm_run(loss_kind=0)"] + READ + ["conv_step"]),
}


def calibrate(monkeypatch, make, attrs):
    """One layer through ptq behind a Recorder: (conv, recorder)."""
    import efficientq_amd.qconv as Q
    conv, x = make_layer(**make)
    for k, v in attrs.items():
        setattr(conv, k, v)
    conv.to(DEV)
    conv.output_fp = conv.output_fp.to(DEV)
    if conv.mask_pyramid:
        conv.mask_pyramid = [m.to(DEV) for m in conv.mask_pyramid]
    rec = record(monkeypatch, Q.get_ops(torch.device(DEV)))
    conv.set_quantizing()
    with torch.no_grad():
        conv(x.to(DEV))
    torch.cuda.synchronize()
    return conv, rec


@pytest.mark.parametrize("name", list(LAYERS))
def test_paths_and_call_sequence_of_the_layer_classes(monkeypatch, name):
    make, attrs, paths, calls = LAYERS[name]
    conv, rec = calibrate(monkeypatch, make, attrs)
    assert conv.last_trace["paths"] == paths
    assert rec.calls == calls
    assert rec.reduced == 2               # the loss history and the final sums; everything else only when data-parallel
