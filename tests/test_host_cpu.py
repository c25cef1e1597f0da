"""Host logic of the product (qconv / unet / calibrate / config) on the CPU, driven through the
test-only oracle backend (tests/cpu_backend.py) and checked against reference goldens.
Also: the C-ABI library loads and exports every declared symbol (no compute without a GPU)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import cpu_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.array(a)).clone()


# ------------------------------------------------------------------ C ABI
def test_library_exports_every_declared_symbol():
    from efficientq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(effq_\w+|conv3d_\w+)\s*\(", hdr))
    declared -= {"effq_geom", "effq_fp_state"}
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = _lib.load()                      # raises if the .so is missing or a symbol is not exported
    assert lib.effq_version() >= 100
    assert lib.effq_reduce_ws_bytes() > 0


def test_solver_dispatch_queries_launch_nothing():
    """effq_prox_plan_query / effq_spd_inverse_plan answer without a device: the classes tests/test_solver_shapes_gpu.py
    pins its cases to (the same prox_plan and the same block threshold the solver calls)."""
    import ctypes as C
    from efficientq_amd import _lib
    lib = _lib.load()

    def prox(c2, n):
        out = [C.c_int() for _ in range(4)]
        assert lib.effq_prox_plan_query(c2, n, *[C.byref(o) for o in out]) == 0
        return tuple(o.value for o in out)

    def inverse(n):
        out = [C.c_int() for _ in range(3)]
        assert lib.effq_spd_inverse_plan(n, *[C.byref(o) for o in out]) == 0
        return tuple(o.value for o in out)

    # (variant, column tiles, row tiles, K slices): the shipped 1x1x1 layers on variants 0 and 1, the split variant 2,
    # the two sides of the bf16 switch
    assert prox(256, 129) == (0, 3, 1, 1) and prox(512, 257) == (0, 5, 2, 1) and prox(256, 513) == (0, 9, 1, 2)
    assert prox(128, 65) == (1, 2, 1, 1) and prox(64, 1729) == (2, 28, 1, 9) and prox(32, 109) == (3, 1, 1, 1)
    assert prox(256, 1023)[0] == 0 and prox(256, 1024)[0] == 5 and prox(128, 1023)[0] == 1 and prox(128, 1024)[0] == 7
    # (wide, 64-blocks, pivot blocks): the wide sweep starts at 100 blocks
    assert inverse(1) == (0, 1, 1) and inverse(6336) == (0, 99, 99)
    assert inverse(6337) == (1, 100, 25) and inverse(6401) == (1, 101, 26) and inverse(6592) == (1, 103, 26)
    v = C.c_int()
    assert lib.effq_prox_plan_query(0, 5, C.byref(v), C.byref(v), C.byref(v), C.byref(v)) == 1      # EFFQ_ERR_ARG
    assert lib.effq_spd_inverse_plan(0, C.byref(v), C.byref(v), C.byref(v)) == 1


def test_gram_dispatch_queries_launch_nothing():
    """effq_gram_plan_query / effq_gram_i8_plan_query / effq_gram_f64_plan_query answer without a device: the classes
    tests/test_gram_shapes_gpu.py pins its cases to (the planners the launches call).  The clamp on the chunks per split of
    the i8 Gram keeps the int32 partial sums of a split in range at the largest level id, whatever the geometry."""
    import ctypes as C
    from efficientq_amd import _lib
    from efficientq_amd.hip_ops import make_geom
    lib = _lib.load()

    def gram(shape, c2, k, s, p, bias):
        g = make_geom(shape, c2, k, s, p)
        out = [C.c_int() for _ in range(4)]
        vps, tail = C.c_longlong(), [C.c_int(), C.c_int()]
        assert lib.effq_gram_plan_query(C.byref(g), bias, *[C.byref(o) for o in out], C.byref(vps),
                                        *[C.byref(o) for o in tail]) == 0
        return tuple(o.value for o in out) + (vps.value,) + tuple(o.value for o in tail)

    def gram_i8(shape, c2, k, ncls=1, n_list=0):
        g = make_geom(shape, c2, k, 1, k // 2)
        out = [C.c_int() for _ in range(6)]
        rc = lib.effq_gram_i8_plan_query(C.byref(g), ncls, n_list, *[C.byref(o) for o in out])
        return (rc,) + tuple(o.value for o in out)

    def gram_f64(shape, c2, k, s, p, bias):
        g = make_geom(shape, c2, k, s, p)
        out = [C.c_int() for _ in range(4)]
        rc = lib.effq_gram_f64_plan_query(C.byref(g), bias, *[C.byref(o) for o in out])
        return (rc,) + tuple(o.value for o in out)

    # (vec, NB, npairs, nsplit, voxels per split, fold, finish blocks)
    assert gram((1, 4, 102, 102, 101), 32, 3, 1, 1, 1) == (1, 2, 3, 1314, 800, 4, 61)          # fold 4 from 2^20 voxels
    assert gram((2, 6, 9, 10, 11), 2, 3, 1, 1, 1) == (0, 2, 3, 7, 288, 1, 106)                 # row-by-row staging
    assert gram((1, 128, 12, 13, 14), 128, 3, 1, 1, 1) == (1, 29, 435, 8, 288, 1, 8192)        # strided finish
    assert gram((1, 4, 6, 8, 9), 8, 3, 1, 1, 1)[3] == 1
    # (rc, NB, NBX, npairs, nchunks, cps, nsplit)
    assert gram_i8((4, 32, 64, 64, 64), 32, 3) == (0, 8, 7, 35, 8192, 94, 88)
    assert gram_i8((1, 16, 128, 128, 128), 16, 1) == (0, 1, 1, 1, 16384, 6, 2731)
    assert gram_i8((1, 32, 8, 8, 8), 32, 3, 16, 1024)[4] == 8                                  # the list sets the chunks
    longest = 0
    for c1, c2, k in [(16, 16, 1), (32, 32, 3), (64, 64, 3), (128, 128, 3), (256, 256, 3), (512, 512, 3), (256, 128, 1)]:
        for nchunks in (1, 4, 4095, 65536, 3072 * 1000, (1 << 24) - 1):
            rc, _, _, _, got, cps, nsplit = gram_i8((1, c1, 8, 8, 8), c2, k, 1, nchunks * 128)
            assert rc == 0 and got == nchunks and cps * nsplit >= nchunks and nsplit <= 65535
            longest = max(longest, cps)
    assert longest == 1000 and longest * 128 * 127 * 127 < 2 ** 31                             # GI_MAX_CPS, 128 levels
    assert gram_i8((1, 16, 8, 8, 8), 16, 1, 1, 130)[0] == 1 and gram_i8((1, 16, 8, 8, 8), 16, 1, 17, 0)[0] == 1
    # (rc, nchunk, grid, ntiles, tiles per wave)
    assert gram_f64((1, 32, 32, 32, 33), 3, 1, 1, 0, 1) == (0, 1056, 1024, 9, 3)
    assert gram_f64((3, 2, 60, 60, 41), 16, 3, (2, 2, 1), 0, 1) == (0, 3075, 1024, 14, 6)
    assert gram_f64((1, 4, 46, 47, 47), 32, 3, 1, 1, 1) == (0, 3176, 1024, 42, 11)
    assert gram_f64((2, 127, 10, 10, 10), 64, 1, 1, 0, 1) == (0, 63, 63, 68, 18)
    # both sides of every step of the ladder (1^3 layers without bias: n = C1)
    for c1, c2, want in [(40, 32, (12, 3)), (64, 16, (14, 6)), (64, 48, (22, 6)), (80, 32, (25, 11)), (128, 16, (44, 11)),
                         (96, 64, (45, 18)), (128, 64, (68, 18))]:
        assert gram_f64((1, c1, 4, 4, 4), c2, 1, 1, 0, 0)[3:] == want, (c1, c2)
    assert gram_f64((1, 32, 8, 8, 8), 32, 3, 1, 1, 1)[0] == 1                                   # n = 865: not supported
    # digit planes of the i8 loss: P balanced digits hold 127 (256^P - 1) / 255, which is below 2^(8P-1) - 1 from P = 2 on
    for P in range(1, 7):
        cap = 127 * ((256 ** P - 1) // 255)
        assert lib.effq_gram_loss_i8_num_planes(cap) == P
        assert lib.effq_gram_loss_i8_num_planes(cap + 1) == (P + 1 if P < 6 else -1)


def test_conv_dispatch_queries_answer_the_classes_of_the_geometry_cases():
    """effq_conv_plan_query / effq_conv_i8_plan_query / effq_conv_i8s_plan_query answer without a device, from the planners
    and the kernel choice the launches use: every case of tests/test_conv_geometry_gpu.py lands in the class it names, and
    the two halo refusals are make_plan's own error."""
    import math
    from efficientq_amd import _lib
    from efficientq_amd import hip_ops as H
    from tests import test_conv_geometry_gpu as G
    lib = _lib.load()
    n = G.N
    for case, (c1, c2, k, s, p, sp, want) in G.F32_TILED.items():
        geom = H.make_geom((n, c1, *sp), c2, k, s, p)
        G.assert_tiled_plan(H.conv_plan_query(lib, geom, False), want)
        assert H.conv_plan_query(lib, geom, True)["kind"] == 0, case
    # every plan branch the cases were written for is there
    plans = {c: H.conv_plan_query(lib, H.make_geom((n, v[0], *v[5]), v[1], v[2], v[3], v[4]), False)
             for c, v in G.F32_TILED.items()}
    big = [c for c, pl in plans.items() if pl["lds_bytes"] > 64 * 1024]
    assert any(plans[c]["nslab"] > 1 for c in big) and any(plans[c]["nslab"] == 1 for c in big)
    assert {pl["cslab"] for pl in plans.values()} == {8, 16, 32} and any(pl["grid_y"] == 3 for pl in plans.values())
    assert all(pl["lds_bytes"] <= 160 * 1024 for pl in plans.values())
    for case, (c1, c2, k, s, p, nn, sp, kernel) in G.DIRECT.items():
        geom = H.make_geom((nn, c1, *sp), c2, k, s, p)
        G.assert_direct_plan(case, H.conv_plan_query(lib, geom, True))
        assert H.conv_plan_query(lib, geom, False)["kind"] == 0, case
    assert {v[7] for v in G.DIRECT.values()} == set(H.CONV_KINDS[1:])
    for case, (c1, c2, k, s, p, sp) in G.F32_REFUSED.items():
        geom = H.make_geom((n, c1, *sp), c2, k, s, p)
        for lo in (False, True):
            with pytest.raises(_lib.EffqError, match=r"EFFQ_ERR_ARG.*halo tile of \d+ voxels does not fit LDS"):
                H.conv_plan_query(lib, geom, lo)
        assert lib.effq_conv_ws_bytes(geom) == 0
    for case, (c1, c2, out, pad, la, lw, _, kern) in list(G.I8.items()) + list(G.I8_FORWARD.items()):
        geom = H.make_geom((n, c1, *G._i8_in(out, pad)), c2, 3, 1, pad)
        assert geom.out_dims() == out and lib.effq_conv_i8_supported(geom, la, lw) == 1, case
        fwd = case in G.I8_FORWARD
        plan = H.conv_i8_plan_query(lib, geom, fwd)
        assert plan["kernel"] == kern and 0 < plan["grid_x"] <= plan["ntiles"], (case, plan)
        if kern not in ("l2e", "i8w"):
            with pytest.raises(_lib.EffqError, match="output"):
                H.conv_i8_plan_query(lib, geom, True)
    assert {v[7] for v in G.I8.values()} == set(H.CONV_I8_KERNELS[1:])
    with pytest.raises(_lib.EffqError):
        H.conv_i8_plan_query(lib, H.make_geom((n, 48, 6, 6, 10), 32, 3, 1, 1), False)
    for case, (c1, c2, k, s, p, la, lw, sp, want) in G.I8S.items():
        geom = H.make_geom((n, c1, *sp), c2, k, s, p)
        G.assert_i8s_plan(H.conv_i8s_plan_query(lib, geom, la, lw), want, c1, k)
    with pytest.raises(_lib.EffqError):
        H.conv_i8s_plan_query(lib, H.make_geom((n, 32, 8, 8, 8), 32, 3, 1, 1), 4, 4)              # K = 864
    # the shipped first convs and the classifier keep their kernels
    for shape, c2, k, s, p, kernel in [((1, 4, 32, 32, 32), 32, 3, 2, 1, "k_conv3d_c4h"), ((1, 4, 32, 32, 32), 32, 3, 1, 1, "k_conv3d_c4h"),
                                       ((1, 1, 32, 32, 32), 32, 3, (2, 2, 1), 1, "k_conv3d_c1h"), ((1, 32, 8, 8, 8), 3, 1, 1, 0, "k_conv1_mfma"),
                                       ((1, 4, 32, 32, 32), 32, 3, (2, 2, 1), 1, "k_conv3d_c4"), ((1, 32, 8, 8, 8), 32, 3, 1, 1, "tiled")]:
        assert H.conv_plan_query(lib, H.make_geom(shape, c2, k, s, p), True)["kernel"] == kernel


def test_conv_comparison_rejects_a_dropped_tap_and_swapped_kernel_axes():
    """The comparison helper of tests/test_conv_geometry_gpu.py can fail.  (a) The fp64 reference of the padding-0 case with
    the largest tap product of one output channel left out at one corner output (all 27 taps there), and the same at the
    padding-(0, 1, 2) case, whose corner has 6 of 27 taps: the elementwise bound rejects both - and so does the max-norm bound
    alone, since an ordinary product is about 1e-1 of the largest output, four orders above 1e-5.  What the elementwise bound
    adds is smaller errors at outputs with a small S: at the 6-tap corner it is 9.7e-6 against the max-norm bound's 2.7e-5, and
    an error between the two is rejected by it alone.  At the 27-tap corner it is the looser one, 7.0e-5 against 2.7e-5: K =
    216, so (K + 2) 2^-24 = 1.3e-5 already exceeds 1e-5, and S there exceeds the largest output.  (b) The (3, 3, 1) case computed with the two kernel axes H and W
    swapped (a (3, 1, 3) kernel on the matching padding): both bounds reject it; an exact copy passes both."""
    import torch.nn.functional as F
    from tests import test_conv_geometry_gpu as G
    for case in ("k3_pad0", "k3_pad012"):
        c1, c2, k, s, p, sp, _ = G.F32_TILED[case]
        pr = G._f32_problem(c1, c2, k, s, p, sp)
        ref, S, K = pr["ref"], pr["S"], pr["K"]
        assert G.value_report(ref.clone(), ref, S, K)[:2] == (True, True)
        pd, ph, pw = G._triple(p)
        # corner output (0, 0, 0) of channel 0, batch 1: its taps are x[1, c, kd - pd, kh - ph, kw - pw] w[0, c, kd, kh, kw]
        prods = {}
        for c in range(c1):
            for kd in range(3):
                for kh in range(3):
                    for kw in range(3):
                        i = (kd - pd, kh - ph, kw - pw)
                        if min(i) >= 0:
                            prods[(c, kd, kh, kw)] = pr["x"][1, c, i[0], i[1], i[2]].double() * pr["w"][0, c, kd, kh, kw].double()
        assert len(prods) == c1 * (27 if case == "k3_pad0" else 6)
        assert abs(sum(prods.values()) + pr["b"][0].double() - ref[1, 0, 0, 0, 0]) <= 1e-12
        got = ref.clone()
        got[1, 0, 0, 0, 0] -= max(prods.values(), key=abs)
        maxnorm_ok, elem_ok, worst = G.value_report(got, ref, S, K)
        assert not elem_ok and worst > 1e3 and not maxnorm_ok
        with pytest.raises(AssertionError, match="max-norm"):
            G.check_values(got, ref, S, K)
        if case == "k3_pad012":
            eb = (K + 2) * 2.0 ** -24 * S[1, 0, 0, 0, 0].item()
            mb = 1e-5 * ref.abs().max().item()
            assert eb < 0.9 * mb, (eb, mb)
            got = ref.clone()
            got[1, 0, 0, 0, 0] += (eb * mb) ** 0.5
            assert G.value_report(got, ref, S, K)[:2] == (True, False)
            with pytest.raises(AssertionError, match="elementwise"):
                G.check_values(got, ref, S, K)
    c1, c2, k, s, p, sp, _ = G.F32_TILED["k331_not_cubic"]
    assert k == (3, 3, 1) and p == (1, 1, 0)
    pr = G._f32_problem(c1, c2, k, s, p, sp)
    swapped = F.conv3d(pr["x"].double(), pr["w"].double().transpose(3, 4), pr["b"].double(), s, (1, 0, 1))
    assert swapped.shape == pr["ref"].shape                       # a 1-wide axis at padding 0 on either side: same output
    maxnorm_ok, elem_ok, _ = G.value_report(swapped, pr["ref"], pr["S"], pr["K"])
    assert not maxnorm_ok and not elem_ok


def test_gram_test_reference_agrees_with_the_oracle():
    """The fp64 slab reference of tests/test_gram_shapes_gpu.py (strided views, slab by slab) against the oracle's
    patch_matrix and ProxSystem at two small shapes - one strided, one without bias - to 1e-12 of the largest entry."""
    from oracle import effq_oracle as O
    from tests.test_gram_shapes_gpu import gram_reference
    for (N, c1, D, H, W), c2, k, s, p, bias in [((2, 3, 7, 8, 9), 5, (3, 3, 3), (2, 2, 1), (1, 1, 1), True),
                                                ((2, 4, 6, 5, 7), 3, (3, 3, 3), (1, 1, 1), (0, 0, 0), False)]:
        gen = torch.Generator().manual_seed(c1 + c2)
        x = torch.randn(N, c1, D, H, W, generator=gen, dtype=torch.float64)
        w = torch.randn(c2, c1, *k, generator=gen, dtype=torch.float64)
        b = torch.randn(c2, generator=gen, dtype=torch.float64) if bias else None
        y = torch.nn.functional.conv3d(x, w, b, s, p) + torch.randn(1, dtype=torch.float64, generator=gen)
        att = torch.randint(1, 4, y[:, 0].shape, generator=gen).double()
        ref = gram_reference(x.permute(0, 2, 3, 4, 1), y.permute(0, 2, 3, 4, 1), att, k, s, p, bias, slab=40,
                             want_patches=True, want_abs=True, G=w, b=b)
        X = O.patch_matrix(x.numpy(), k, s, p, ones_row=bias, dtype=np.float64)
        assert np.array_equal(ref["patches"].numpy(), X.T) and ref["V"] == X.shape[1] and ref["n"] == X.shape[0]
        ps = O.ProxSystem(x, y, k, s, p, w, b, att, dtype=torch.float64)
        Y = y.permute(1, 0, 2, 3, 4).reshape(c2, -1)
        for got, want in ((2 * ref["A"], ps.A0), (2 * ref["B"], ps.B0), (ref["Au"], T(X @ X.T)), (ref["Bu"], Y @ T(X).T),
                          (ref["absA"], T(np.abs(X) @ np.abs(X).T))):
            assert (got - want).abs().max() <= 1e-12 * want.abs().max()
        out = torch.nn.functional.conv3d(x, w, b, s, p)
        assert abs(ref["loss"] - ((out - y) ** 2).sum().item()) <= 1e-12 * ((out - y) ** 2).sum().item()


def test_product_path_refuses_cpu_tensors():
    from efficientq_amd import hip_ops, _lib
    with pytest.raises(_lib.EffqError):
        hip_ops.get_ops("cpu")
    from efficientq_amd.qconv import EfficientQConvHIP
    conv = EfficientQConvHIP(2, 2, 3, 1, 1)
    with pytest.raises(_lib.EffqError):
        conv(torch.zeros(1, 2, 4, 4, 4))


def _admm_args(lib, c2=8, c1=3, k=3, **fields):
    """An effq_admm_run argument block for a c2 x c1 x k^3 layer with bias that passes every check, then `fields`.
    The pointers are dummies: every case below is rejected before the run touches a device."""
    from efficientq_amd import _lib
    a = _lib.AdmmRunArgs()
    dummy = 1 << 20
    for name in ("A0", "B0", "W0", "b0", "xq", "y_fp", "dual", "wstar", "v", "G_ring", "b_ring", "state_ring", "hist",
                 "err_flag", "ainv_pool", "prox_ws", "red_ws", "inv_ws", "conv_ws"):
        setattr(a, name, dummy)
    a.c2, a.n, a.has_bias, a.w_levels = c2, c1 * k ** 3 + 1, 1, 4
    a.iters, a.rho_period, a.rho, a.rho_max, a.eta, a.tol = 10, 2, 0.5, 4.0, 1e-3, 1e-6
    a.geom = _lib.Geom(1, c1, c2, 4, 4, 4, k, k, k, 1, 1, 1, k // 2, k // 2, k // 2)
    a.loss_kind, a.act_levels = 0, 4
    a.n_ainv = lib.effq_admm_num_inverses(a.rho, a.rho_max, a.iters, a.rho_period)
    for name, value in fields.items():
        setattr(a, name, dummy if value is ... else value)   # ... = a dummy pointer
    return a


_ADMM_REJECTS = [   # (case, arguments, expected status, the part of effq_last_error() that names the check)
    ("null args", None, "EFFQ_ERR_ARG", "a != nullptr"),
    ("loss kind 3", dict(loss_kind=3), "EFFQ_ERR_ARG", "a->loss_kind == 4 || a->loss_kind == 5"),
    ("loss kind 4 without its Gram operands", dict(loss_kind=4), "EFFQ_ERR_ARG",
     "a->loss_Au != nullptr && a->loss_Bu != nullptr && a->loss_syy != nullptr"),
    ("channel mode with loss kind 1", dict(channel_wise=1, alpha_ring=..., loss_kind=1, xidx=..., Gq_ring=...,
                                           act_alpha_dev=...), "EFFQ_ERR_ARG",
     "(a->loss_kind == 0 || a->loss_kind == 4) && a->alpha_ring != nullptr"),
    ("weights that do not match geom", dict(n=83), "EFFQ_ERR_ARG", "a->geom.C2 * a->geom.C1"),
    ("weights above effq_fp_coop_max", "coop", "EFFQ_ERR_ARG", "exceed the single-launch fixed points"),
    ("bucketed fixed-point workspace too small", dict(c2=64, fp_ws=..., fp_ws_bytes=0), "EFFQ_ERR_WORKSPACE",
     "admm_run: fixed-point workspace 0 <"),
    ("trajectory workspace too small", dict(c2=810, fp_pred=..., fp_traj_ws=..., fp_traj_ws_bytes=0),
     "EFFQ_ERR_WORKSPACE", "trajectory fixed-point workspace 0 <"),
    ("n_ainv below effq_admm_num_inverses", "n_ainv", "EFFQ_ERR_ARG", "a->n_ainv >="),
]


def _admm_rejections():
    """Child process of admm_rejections: every case of _ADMM_REJECTS, as one JSON line {case: [status, message]}."""
    import ctypes
    import json
    from efficientq_amd import _lib
    assert torch.cuda.device_count() == 0, "a device is visible: the dummy pointers must never reach one"
    lib = _lib.load()
    out = {}
    for case, args, _, _ in _ADMM_REJECTS:
        if args is None:
            rc = lib.effq_admm_run(None)
        else:
            if args == "coop":
                a = _admm_args(lib, c2=lib.effq_fp_coop_max() // 81 + 1, k=1, c1=81)
                assert a.c2 * (a.n - 1) > lib.effq_fp_coop_max()
            elif args == "n_ainv":
                a = _admm_args(lib)
                a.n_ainv -= 1
                assert a.n_ainv >= 1
            else:
                a = _admm_args(lib, **args)
            nw = a.c2 * (a.n - 1)
            if a.fp_ws:               # the case is the bucketed path's ...
                assert 4096 < nw <= 1 << 19 and lib.effq_fp_bucket_ws_bytes(nw) > 0
            if a.fp_traj_ws:          # ... and the trajectory path's
                assert lib.effq_admm_uses_traj(nw, a.w_levels) == 1 and lib.effq_fp_traj_ws_bytes(nw) > 0
            rc = lib.effq_admm_run(ctypes.byref(a))
        out[case] = [_lib._ERR_NAMES.get(rc, rc), lib.effq_last_error().decode()]
    print(json.dumps(out))


@pytest.fixture(scope="module")
def admm_rejections():
    """Runs the cases in a child process that sees no device: a check that stopped rejecting would fail there with
    EFFQ_ERR_HIP instead of writing through a dummy pointer on a real card."""
    import json
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", "from tests.test_host_cpu import _admm_rejections; _admm_rejections()"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case,want,check", [(c, w, m) for c, _, w, m in _ADMM_REJECTS],
                         ids=[c[0] for c in _ADMM_REJECTS])
def test_admm_run_rejects_bad_arguments_before_any_device_call(admm_rejections, case, want, check):
    status, message = admm_rejections[case]
    assert status == want and check in message, (status, message)


# ------------------------------------------------------------------ graph / state_dict / BN fold / masks
def _tiny(task, L=4, width=None, init_stride=None):
    from efficientq_amd import config as Cf
    base = dict(Cf.TINY_NET, width=width) if width else Cf.TINY_NET
    if init_stride:
        base = dict(base, init_stride=init_stride)
    if task == "lits":
        args = Cf.make_args(base, L, L, lwq_batchsz=2)
    else:
        net = dict(base, task="brats", nMod=2, nClass=4, multi_label="brats", init_stride="2,2,2")
        args = Cf.make_args(net, L, L, lwq_batchsz=2)
    QConv, info, kwQ = Cf.get_conv_class(args)
    cube, _ = Cf.get_model_cube(args, QConv, kwQ)
    return args, cube["model"], info


@pytest.mark.parametrize("task,fname", [("lits", "g6_tiny_lits_L4.npz"), ("brats", "g6_tiny_brats_L4.npz")])
def test_state_dict_keys_match_reference(gold, task, fname):
    g = gold(fname)
    args, model, info = _tiny(task)
    want = {k[4:]: g[k].shape for k in g.files if k.startswith("sd0/")}
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert set(got) == set(want)
    assert all(tuple(want[k]) == got[k] for k in want)
    assert info == "effq_bothQw4a4"


def test_full_size_nets_have_the_surveyed_layer_counts():
    from efficientq_amd import config as Cf
    from efficientq_amd.qconv import PTQConv
    for net, nq, npar in ((Cf.BRATS_NET, 22, 5.96e6), (Cf.LITS_NET, 28, 23.9e6)):
        args = Cf.make_args(net, 4, 4)
        QConv, _, kwQ = Cf.get_conv_class(args)
        model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
        qs = [m for m in model.modules() if isinstance(m, PTQConv)]
        assert len(qs) == nq
        assert abs(sum(p.numel() for p in model.parameters()) - npar) / npar < 0.02
        assert qs[0].qlvl_w == 256 and not qs[0].q_act and qs[-1].qlvl_w == 256 and not qs[-1].q_act
        assert qs[1].qlvl_w == 4 and qs[1].q_act and qs[1].qlvl_act == 4


def test_bn_fold_matches_reference(gold):
    from efficientq_amd.unet import ConvUnit
    from efficientq_amd.calibrate import search_fold_and_remove_bn
    g = gold("g7_bnfold.npz")
    blk = ConvUnit("mid", 4, 6, 3, 1, 1, 1, nn.Conv3d, nn.BatchNorm3d, True, 0)
    with torch.no_grad():
        blk.conv.weight.copy_(T(g["w"]))
        blk.bn.weight.copy_(T(g["gamma"])); blk.bn.bias.copy_(T(g["beta"]))
        blk.bn.running_mean.copy_(T(g["mean"])); blk.bn.running_var.copy_(T(g["var"]))
    blk.eval()
    assert torch.equal(blk(T(g["x"])), T(g["y_before"]))
    search_fold_and_remove_bn(blk)
    assert torch.equal(blk.conv.weight.data, T(g["w_fold"]))
    assert torch.equal(blk.conv.bias.data, T(g["b_fold"]))
    assert torch.equal(blk(T(g["x"])), T(g["y_after"]))


def test_resunit_inplace_relu_residual(gold):
    from efficientq_amd.unet import ResUnit
    g = gold("g10_resblock_mid.npz")
    rb = ResUnit("mid", 4, 4, 0.5, 1, nn.Conv3d, nn.BatchNorm3d)
    rb.load_state_dict({k[3:]: T(g[k]) for k in g.files if k.startswith("sd/")})
    rb.eval()
    assert torch.equal(rb(T(g["x"])), T(g["y"]))


@pytest.mark.parametrize("task", ["lits", "brats"])
def test_attention_masks_match_reference(gold, task):
    from efficientq_amd import calibrate as K
    g = gold("g8_attmask.npz")
    for key, st in ((f"{task}_s1", "1"), (f"{task}_s2", "2,2,2"), (f"{task}_s221", "2,2,1")):
        logits, data = T(g[f"{key}_logits"]), T(g[f"{key}_data"])
        ones = torch.ones_like(data[:, 0]).bool()
        body = (data[:, 0] != 0).bool() if task == "brats" else ones
        wmap, nums = K.get_att_weight_map(logits, ones, "p:0.5", task=task)
        assert nums == g[f"{key}_nums"].tolist()
        assert [wmap[i] for i in range(len(wmap))] == g[f"{key}_wvals"].tolist()
        pyr = K.get_mask_pyramid(logits, body, wmap, st, num_lvls=3, task=task)
        for i, m in enumerate(pyr):
            assert torch.equal(m, T(g[f"{key}_pyr{i}"]).float())


def test_int_weight_storage_roundtrip(gold):
    from efficientq_amd.qconv import PTQConv
    g = gold("g9_intweight.npz")
    for L in (4, 16, 256):
        conv = PTQConv(4, 6, 3, 1, 1, qlvl=L)
        conv.weight.data = T(g[f"L{L}_q"])
        conv.alpha_w.data = T(g[f"L{L}_alpha"])
        conv.store_int_weight()
        assert conv.weight.data.dtype == torch.uint8 and torch.equal(conv.weight.data, T(g[f"L{L}_int"]))
        conv.restore_fp_weight()
        assert torch.equal(conv.weight.data, T(g[f"L{L}_restored"]))


def test_center_crop_pads_and_crops():
    from efficientq_amd.calibrate import center_crop
    t = torch.arange(2 * 5 * 6 * 7, dtype=torch.float32).reshape(2, 5, 6, 7)
    c = center_crop(t, (3, 4, 5))
    assert torch.equal(c, t[:, 1:4, 1:5, 1:6])
    p = center_crop(t, (8, 6, 7))
    assert p.shape == (2, 8, 6, 7) and torch.equal(p[:, 1:6], t) and p[:, 0].abs().sum() == 0


# ------------------------------------------------------------------ layer calibration through the product's ptq()
def _layer_from_gold(g, tag):
    from efficientq_amd.qconv import EfficientQConvHIP
    c1, c2, k, pad, N, S, L_w, L_a, q_act, with_mask = [int(v) for v in g[f"{tag}_meta"]]
    stride = tuple(int(v) for v in g[f"{tag}_stride"])
    conv = EfficientQConvHIP(c1, c2, k, stride, pad, 1, 1, True, q_weight=True, qlvl=L_w, q_act=bool(q_act),
                             qlvl_act=L_a)
    conv.weight.data = T(g[f"{tag}_w_in"])
    conv.bias.data = T(g[f"{tag}_b_in"])
    conv.output_fp = T(g[f"{tag}_y"])
    conv.name = "layer"
    conv.layer_loss = []
    if with_mask:
        y = conv.output_fp
        conv.mask_pyramid = [torch.ones(N, *[d // 2 for d in y.shape[2:]]), T(g[f"{tag}_mask_full"])]
    return conv, T(g[f"{tag}_x"]), (L_w, L_a, bool(q_act))


def _progress_lines(text):
    import re
    pat = re.compile(r"ADMM iter (\d+): primal residual = ([0-9.]+), dual residual = ([0-9.]+), rho = ([0-9.]+), "
                     r"eta = ([0-9.]+), loss = ([0-9.]+)\.")
    return [(int(m[1]), float(m[2]), float(m[3]), float(m[4]), float(m[5]), float(m[6])) for m in pat.finditer(text)]


def test_lwq_verbose_prints_the_reference_progress_line(gold, monkeypatch, capsys):
    """EfficientQConv.py:114-127: 'ADMM iter i+1: primal residual = ..., dual residual = ..., rho = ..., eta = ..., loss = ...'
    every 10 iterations, with ||w* - G||, rho ||G - G0|| and the iteration's MSE - against the oracle's histories."""
    import oracle.effq_oracle as O
    cpu_backend.install(monkeypatch)
    g = gold("g5_layer_ptq.npz")
    conv, x, (L_w, L_a, q_act) = _layer_from_gold(g, "L4")
    conv.lwq_verbose = True
    conv.set_quantizing()
    with torch.no_grad():
        conv(x)
    lines = _progress_lines(capsys.readouterr().out)
    assert [l[0] for l in lines] == list(range(1, 200, 10))
    c1, c2, k, pad, N, S, _, _, _, with_mask = [int(v) for v in g["L4_meta"]]
    ref = O.calibrate_layer(x, T(g["L4_y"]), T(g["L4_w_in"]), T(g["L4_b_in"]), tuple(int(v) for v in g["L4_stride"]), pad,
                            qlvl_w=L_w, qlvl_act=L_a, q_act=q_act, mask_pyramid=conv.mask_pyramid if with_mask else None)
    for it, pres, dres, rho, eta, loss in lines:
        i = it - 1
        assert abs(rho - ref.rho_history[i]) <= 1e-4 * ref.rho_history[i] + 1e-4
        assert abs(pres - ref.primal_res[i]) <= 2e-3 * ref.primal_res[i] + 5e-3, (i, pres, ref.primal_res[i])
        assert abs(dres - ref.dual_res[i]) <= 2e-3 * ref.dual_res[i] + 5e-3, (i, dres, ref.dual_res[i])   # (late: a flip or none)
        assert abs(loss - ref.loss_history[i]) <= 1e-3 * ref.loss_history[i] + 1e-7


@pytest.mark.parametrize("tag", ["L4", "L16", "first", "k1"])
def test_product_ptq_on_oracle_backend_matches_reference(gold, monkeypatch, tag):
    cpu_backend.install(monkeypatch)
    g = gold("g5_layer_ptq.npz")
    conv, x, (L_w, L_a, q_act) = _layer_from_gold(g, tag)
    conv.set_quantizing()
    with torch.no_grad():
        out = conv(x)
    want_loss = float(g[f"{tag}_layer_loss"])
    got_loss = float(conv.layer_loss[0].split(":")[1])
    assert abs(got_loss - want_loss) <= 1e-6 * want_loss
    assert conv.layer_loss[0].startswith(f"{'layer':45s}:")
    # the stand-in's conv runs on channels-last memory, so the per-iteration losses differ in the last
    # ulp and the best iterate may be another point of the same plateau: indices must agree
    # exactly, values to fp32 rounding
    wg = T(g[f"{tag}_weight"])
    lv = lambda t: torch.round((t / t.abs().max() + 1) * (L_w - 1) / 2)
    assert torch.equal(lv(conv.weight.data), lv(wg))
    assert (conv.weight.data - wg).abs().max() <= 2e-6 * wg.abs().max()
    assert (conv.bias.data - T(g[f"{tag}_bias"])).abs().max() <= 1e-3 * T(g[f"{tag}_bias"]).abs().max()  # b* of another plateau iterate
    assert abs(conv.alpha_w.data.item() - float(g[f"{tag}_alpha_w"])) <= 2e-6 * float(g[f"{tag}_alpha_w"])
    if q_act:
        assert conv.alpha_act.data.item() == float(g[f"{tag}_alpha_act"])
    assert (out - T(g[f"{tag}_fwd_q"])).abs().max() <= 1e-4 * T(g[f"{tag}_fwd_q"]).abs().max()


# ------------------------------------------------------------------ whole do_ptq window on the tiny nets
def _run_tiny(task, fname, gold, monkeypatch):
    from efficientq_amd import calibrate as K
    cpu_backend.install(monkeypatch)
    # g6_*: the reference run on the CPU, where its hook's `.cpu()` aliases the conv output and the next in-place ReLU
    # overwrites half of the targets; g6c_*: the same run with the copy a GPU run makes (make_goldens._copying_hook)
    monkeypatch.setattr(K, "ALIAS_FP_TARGETS", not fname.startswith("g6c"))
    g = gold(fname)
    args, model, _ = _tiny(task)
    model.load_state_dict({k[4:]: T(g[k]) for k in g.files if k.startswith("sd0/")}, strict=False)
    model.eval()
    K.search_fold_and_remove_bn(model)
    S = int(g["meta"][1])
    nmod = 1 if task == "lits" else 2
    vols = torch.randn(2, nmod, S, S, S, generator=torch.Generator().manual_seed(int(g["vols_seed"])))
    if task == "brats":
        zz = torch.arange(S).float() - (S - 1) / 2
        r = (zz[:, None, None] ** 2 + zz[None, :, None] ** 2 + zz[None, None, :] ** 2).sqrt()
        vols = vols * (r < 0.45 * S).float()
    assert torch.equal(vols[:, :, ::8, ::8, ::8], T(g["vols_check"]))
    K.set_name(model)
    res = K.calibrate_model(model, vols, task, args.init_stride)
    return g, model, res


@pytest.mark.usefixtures("golden_threads")       # the whole-net run amplifies last-ulp differences layer by layer
@pytest.mark.parametrize("task,fname", [("brats", "g6_tiny_brats_L4.npz"), ("brats", "g6c_tiny_brats_L4.npz")])
def test_whole_calibration_on_oracle_backend_matches_reference(gold, monkeypatch, task, fname):
    g, model, res = _run_tiny(task, fname, gold, monkeypatch)
    names = [l.split(":")[0].strip() for l in res["layer_loss"]]
    assert names == g["layer_names"].tolist()
    got = np.array([float(l.split(":")[1]) for l in res["layer_loss"]])
    assert res["nums"] == g["class_nums"].tolist()
    for i, m in enumerate(res["pyramid"]):
        assert torch.equal(m, T(g[f"pyr{i}"]).float())
    # Layer-level parity (1e-3 relative MSE on IDENTICAL inputs) is pinned by the g5 tests above.  In the
    # whole-net run each layer is calibrated on the quantised upstream's output, so once one layer keeps a
    # different iterate of its loss plateau (last-ulp loss differences) the inputs of all later layers
    # differ and their losses drift at the percent level, in both directions (hard parts).
    want = g["layer_loss"]
    assert np.all(np.abs(got[:3] - want[:3]) <= 1e-5 * want[:3]), (got, want)
    # (the copy-semantics run drifts a little more on its late layers: 9 % on one of them, towards either side)
    drift, total = (1.2e-1, 5e-2) if fname.startswith("g6c") else (5e-2, 3e-2)
    assert np.all(np.abs(got - want) <= drift * want), (got, want)
    assert abs(got.sum() - want.sum()) <= total * want.sum()
    sub = (slice(None), slice(None), slice(None, None, 4), slice(None, None, 4), slice(None, None, 4))
    assert torch.allclose(res["output_fp"][-1][sub], T(g["output_fp_sub"]), atol=1e-5)
    oq, oq_ref = res["output_q"][-1][sub], T(g["output_q_sub"])
    assert ((oq - oq_ref) ** 2).mean() <= 2e-2 * (oq_ref ** 2).mean()
    # model-level agreement of the quantised with the FP prediction (Dice proxy) within 0.5 pt
    agree = ((res["output_q"][-1] > 0) == (res["output_fp"][-1] > 0)).float().mean().item()
    assert abs(agree - float(g["agree"])) <= 5e-3
    sd = model.state_dict()
    for k in g.files:
        if k.startswith("sdq/") and k.endswith("alpha_w") and ("conv0" in k or "UResBlock1" in k):
            assert abs(sd[k[4:]].item() - float(g[k])) <= 1e-4 * abs(float(g[k])), k


def test_entrance_ptq_with_a_yaml_config_and_yaml_beats_the_command_line(tmp_path, monkeypatch):
    """Row b2: the `entrance.py ptq --config x.yaml` flow (entrance.py:17-28, 116-126).  Every NON-NULL key of the YAML
    replaces the command-line value (quirk Q15: the file wins), null keys leave the command line alone, and keys the
    parser does not know (the reference's configs carry data paths etc.) are simply attached to the namespace.  The
    calibration itself runs on the oracle-backed stand-in (tests/cpu_backend.py), `device: cpu` coming from the YAML."""
    import yaml
    from efficientq_amd import config as Cf, entrance
    cpu_backend.install(monkeypatch)
    snap = str(tmp_path / "snap")
    cfg = dict(task="lits", model="UResQ", nMod=1, nClass=3, init_stride="1", depth="1,1,1", width="8,16,8", nla="relu",
               norm="bn", drop_rate=0.5, ds="simple", hetero_dim=True, blk="mid", init_kernel=3, qconv="effq",
               qlvl_w=4, qlvl_a=4, q_first=None, q_last="256,-1", lwq_batchsz=2, lwq_patchsz="16,16,16", device="cpu",
               synthetic=True, no_test=True, snap_dir=snap, data_dir="/data/lits", split_dir=None, some_new_key=7)
    path = tmp_path / "lits_tiny_ptq.yaml"
    path.write_text(yaml.safe_dump(cfg))
    argv = ["ptq", "--config", str(path), "--qlvl_w", "16", "--qlvl_a", "16", "--width", "4,8,4", "--task", "brats",
            "--q_first", "256,-1", "--q_last", "16,16", "--lwq_batchsz", "1"]
    # the merge on its own
    args = Cf.merge_config(str(path), Cf.build_parser().parse_args(argv))
    assert (args.qlvl_w, args.qlvl_a, args.width, args.task, args.lwq_batchsz) == (4, 4, "8,16,8", "lits", 2)   # YAML wins
    assert args.q_first == "256,-1"              # null in the YAML: the command line's value stays
    assert args.q_last == "256,-1" and args.device == "cpu" and args.some_new_key == 7 and args.split_dir is None
    # and the whole mission
    entrance.main(argv)
    lines = open(os.path.join(snap, "layer_loss.txt")).read().strip().split("\n")
    assert len(lines) == 10 and lines[0].startswith(f"{'conv0.conv':45s}:")
    for f in ("time_cost.txt", "class_voxel_nums.txt", "state_in_fp.pkl", "state_in_int8.pkl", "state_in_int8_compress.npz"):
        assert os.path.exists(os.path.join(snap, f)), f
    sd = torch.load(os.path.join(snap, "state_in_int8.pkl"))["state_dict"]
    w = sd["u_blocks.UResBlock1.Layer1.block1.conv.weight"]
    assert w.dtype == torch.uint8 and int(w.max()) <= 3 and tuple(w.shape[:2]) == (8, 8)      # 4 levels, width 8: the YAML's
    assert int(sd["conv0.conv.weight"].max()) > 3                                             # q_first 256 from the command line


# ------------------------------------------------------------------ data-parallel (gloo, world_size 2)
def test_data_parallel_two_ranks_gloo_matches_single_rank(tmp_path):
    script = os.path.join(ROOT, "tests", "dp_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    out = str(tmp_path / "dp")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29611", script, out],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    single = torch.load(out + "_single.pt")
    dp0, dp1 = torch.load(out + "_rank0.pt"), torch.load(out + "_rank1.pt")
    # replicas stay in lock step: identical weights on both ranks
    for k in dp0["sd"]:
        assert torch.equal(dp0["sd"][k], dp1["sd"][k]), k
    assert dp0["nums"] == single["nums"]
    a, b = np.array(dp0["loss"]), np.array(single["loss"])
    assert np.all(np.abs(a - b) <= 1e-3 * b), (a, b)


def test_registration_shim_with_a_foreign_base_keeps_the_hip_calibrator():
    """the two-line class a maintainer adds to the reference tree - the HIP calibrator with the
    reference's own PTQConv as a second base - is what makes the reference's helpers (isinstance(module, PTQConv))
    see the layers.  The foreign base here is a stand-in nn.Conv3d subclass with a broadcaster that finds layers by
    isinstance, as the reference's do: construction through the product's UResQ factory, MRO, the foreign and the
    product's mode / name / mask broadcasters, state_dict keys, and the HIP `ptq` winning the method lookup."""
    from efficientq_amd import calibrate as K, config as Cf
    from efficientq_amd.qconv import EfficientQConvHIP as Hip

    class ForeignPTQConv(nn.Conv3d):
        def ptq(self, *a, **kw):
            raise NotImplementedError

    def foreign_set_anything(model, attr, value):
        for m in model.modules():
            if isinstance(m, ForeignPTQConv):
                setattr(m, attr, value)

    class EfficientQConvHIP(Hip, ForeignPTQConv):      # the shim of INTEGRATION.md
        pass

    mods = [c.__module__.split(".")[0] for c in EfficientQConvHIP.__mro__[1:4]]
    assert mods == ["efficientq_amd", "efficientq_amd", __name__.split(".")[0]], mods
    assert EfficientQConvHIP.__mro__.index(ForeignPTQConv) < EfficientQConvHIP.__mro__.index(nn.Conv3d)
    args = Cf.make_args(Cf.TINY_NET, 4, 4)
    _, _, kwQ = Cf.get_conv_class(args)
    model = Cf.get_model_cube(args, EfficientQConvHIP, kwQ)[0]["model"]
    q = [m for m in model.modules() if isinstance(m, ForeignPTQConv)]
    assert len(q) == 10 and all(isinstance(m, Hip) for m in q)
    assert q == [m for m in model.modules() if isinstance(m, Hip)]
    K.set_name(model)
    foreign_set_anything(model, "mask_pyramid", ["m"])
    K.set_quantizing(model)
    assert q[0].name == "conv0.conv" and q[0].mask_pyramid == ["m"] and q[0]._quantizing and not q[0]._fp
    K.set_quantized(model)
    assert all(m._quantized for m in q)
    keys = set(model.state_dict())
    assert {"conv0.conv.weight", "conv0.conv.alpha_act", "conv0.conv.alpha_w"} <= keys
    assert type(q[0]).ptq is Hip.ptq                   # the HIP calibrator, not the foreign base's NotImplementedError


def _bench(*flags, env=None, timeout=600):
    e = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], env=e, capture_output=True,
                          text=True, timeout=timeout)


def test_bench_starts_its_own_ranks_for_gpus_above_one():
    """`python bench.py --gpus N` (the driver's command form) must launch N ranks itself, run a real all-reduce over
    them and relay exactly ONE JSON line; here on gloo / CPU, without any calibration (--spawn-check)."""
    import json
    r = _bench("--gpus", "2", "--spawn-check", env={"EFFQ_BENCH_BACKEND": "gloo"})    # whatever GPUs the host has
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2


def test_bench_refuses_a_rank_count_that_differs_from_gpus_and_relays_child_failure():
    # under a launcher (WORLD_SIZE set) --gpus must equal the world size
    r = _bench("--gpus", "4", "--spawn-check", env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr
    # a failing rank makes the parent exit non-zero and print no result line (no GPU here: the ranks cannot calibrate)
    r = _bench("--gpus", "2", "--steps", "1", "--warmup", "0")
    assert r.returncode != 0
    assert not any(l.startswith("{") for l in r.stdout.splitlines())


def test_bench_config_presets():
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    a = bench.parse_args([])
    assert (a.net, a.levels, a.vols, a.size, a.gpus) == ("brats", 4, 16, 128, 1)       # BASELINE configs[1]
    a = bench.parse_args(["--config", "3"])
    assert (a.net, a.levels, a.vols, a.size) == ("brats", 16, 8, 128)                  # configs[2]
    a = bench.parse_args(["--config", "4", "--vols", "2"])
    assert (a.net, a.levels, a.vols, a.size) == ("lits", 4, 2, 160)                    # configs[3], flag override


def test_bench_runs_its_sub_runs_and_the_cpu_baseline_only_with_full():
    """A plain run measures nothing after its timed steps; --full adds the three extra measurements on one GPU, each
    where it applies (exact-integer default path, losses from the Gram system, BraTS net) and unless its flag drops it."""
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    every = ("conv_path", "f32_only", "cpu_baseline")

    def runs(flags, solo=True, exact=True, gram_loss=True):
        return bench.extra_runs(bench.parse_args(flags), solo, exact, gram_loss)

    assert bench.parse_args([]).full is False and bench.parse_args(["--full"]).full is True
    assert runs([]) == () and runs(["--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", "d"]) == ()
    # the flags that leave one out do not bring the others in
    assert runs(["--no-cpu-baseline"]) == () and runs(["--no-f32-subrun", "--no-conv-subrun"]) == ()
    assert runs(["--full"]) == every
    assert runs(["--full", "--no-conv-subrun"]) == every[1:]
    assert runs(["--full", "--no-f32-subrun"]) == (every[0], every[2])
    assert runs(["--full", "--no-cpu-baseline"]) == every[:2]
    assert runs(["--full", "--no-cpu-baseline", "--no-f32-subrun", "--no-conv-subrun"]) == ()
    assert runs(["--full"], solo=False) == ()                          # one rank of several, or not rank 0
    assert runs(["--full"], exact=False) == ("cpu_baseline",)          # the f32 path is already the like-for-like dtype
    assert runs(["--full"], gram_loss=False) == every[1:]              # the losses already come from conv passes
    assert runs(["--full", "--config", "4"]) == every[:2]              # the CPU baseline models the BraTS net only


@pytest.mark.parametrize("tag,psz,ov", [("a", 6, 2), ("b", (6, 12, 6), (2, 0, 3)), ("c", 7, 3)])
def test_sliding_window_helpers_match_reference(gold, tag, psz, ov):
    """Row f1 host logic (efficientq_amd/evaluate.py) against the reference's split / stitch / Dice goldens."""
    from efficientq_amd import evaluate as E
    g = gold("g11_sliding_window.npz")
    img = torch.from_numpy(g[f"{tag}_img"])
    patches = E.image_to_patch3d(img, psz, ov)
    assert torch.equal(torch.stack(patches), torch.from_numpy(g[f"{tag}_patches"]))
    preds = [torch.stack([p * 2.0 + 1.0, p.flip(1) - 0.5]) for p in patches]
    assert torch.equal(E.patch_to_image3d(img, preds, psz, ov), torch.from_numpy(g[f"{tag}_stitched"]))
    # the driver loop over a "model": identity heads give the image back wherever patches agree
    out = E.sliding_window_forward(lambda p: [p, 2 * p], img, psz, ov)
    assert out.shape == (2,) + tuple(img.shape) and torch.allclose(out[0], img, atol=1e-6)
    with pytest.raises(RuntimeError):
        E.image_to_patch3d(img, 64, 2)                      # patch larger than the image
    logits = torch.from_numpy(g["m_logits"])
    d_l = torch.stack([d.float() for d in E.validate_vs_label(logits, torch.from_numpy(g["m_tgt_lits"]), "lits")])
    d_b = torch.stack([d.float() for d in E.validate_vs_label(logits, torch.from_numpy(g["m_tgt_brats"]), "brats")])
    assert torch.equal(d_l, torch.from_numpy(g["m_dice_lits"])) and torch.equal(d_b, torch.from_numpy(g["m_dice_brats"]))


def test_bench_dump_outputs_writes_float_arrays_within_the_size_limit(tmp_path):
    """bench.py --dump-outputs: every result of the step as a float32 / float64 .npy, large outputs sampled at the same
    seeded indices on every call, the calibrated parameters whole, at most 64 MB in all."""
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    from efficientq_amd import config as Cf
    args = Cf.make_args(Cf.TINY_NET, 4, 4)
    QConv, _, kwQ = Cf.get_conv_class(args)
    model = Cf.get_model_cube(args, QConv, kwQ)[0]["model"]
    gen = torch.Generator().manual_seed(0)
    big = torch.randn(bench.DUMP_SAMPLE + 5, generator=gen)
    res = dict(output_fp=[torch.randn(2, 3, 4, generator=gen), big], output_q=[big * 2.0], weight_map=torch.ones(7),
               layer_loss=[f"{'conv0.conv':45s}:0.125", f"{'conv1.conv':45s}:2.5"], nums=[3, 4])
    bench.dump_outputs(str(tmp_path / "a"), res, model)
    bench.dump_outputs(str(tmp_path / "b"), res, model)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(["output_fp_0.npy", "output_fp_1_sample.npy", "output_q_0_sample.npy", "weight_map.npy",
                            "layer_loss.npy", "class_nums.npy", "calibrated_weight.npy", "calibrated_bias.npy",
                            "calibrated_alpha_w.npy", "calibrated_alpha_act.npy"])
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "output_fp_1_sample.npy").size == bench.DUMP_SAMPLE
    assert np.array_equal(np.load(tmp_path / "a" / "output_q_0_sample.npy"),
                          2.0 * np.load(tmp_path / "a" / "output_fp_1_sample.npy"))
    assert np.load(tmp_path / "a" / "layer_loss.npy").tolist() == [0.125, 2.5]
    sd = model.state_dict()
    assert np.load(tmp_path / "a" / "calibrated_weight.npy").size == sum(
        v.numel() for k, v in sd.items() if k.endswith(".weight"))


def test_bench_dump_outputs_samples_the_lits_net_parameters_within_the_size_limit(tmp_path):
    """The LiTS net (--config 4) holds 22.8 M weights, 91 MB in float32: the dump keeps a seeded sample of them and stays
    within 64 MB, and so does a dump with more outputs than the per-array caps leave room for."""
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    _, model = bench.build_model(4, "cpu", "lits")
    n_w = sum(v.numel() for k, v in model.state_dict().items() if k.endswith(".weight"))
    assert n_w > bench.DUMP_PARAM_SAMPLE
    gen = torch.Generator().manual_seed(0)
    out = torch.randn(2 * bench.DUMP_SAMPLE, generator=gen)
    res = dict(output_fp=out, output_q=out * 0.5, weight_map=torch.ones(3), layer_loss=[f"{'c':45s}:1.0"] * 28, nums=[1, 2, 3])
    for tag, r in (("lits", res), ("many", dict(res, output_fp=[out] * 24))):
        for run in ("a", "b"):
            bench.dump_outputs(str(tmp_path / tag / run), r, model)
        files = sorted(p.name for p in (tmp_path / tag / "a").iterdir())
        total = 0
        for n in files:
            x, y = np.load(tmp_path / tag / "a" / n), np.load(tmp_path / tag / "b" / n)
            assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), (tag, n)
            total += x.nbytes
        assert total <= 64 << 20, (tag, total)
        assert "calibrated_weight_sample.npy" in files and "calibrated_bias.npy" in files
        assert np.load(tmp_path / tag / "a" / "layer_loss.npy").size == 28
    assert np.load(tmp_path / "lits" / "a" / "calibrated_weight_sample.npy").size == bench.DUMP_PARAM_SAMPLE
    assert np.load(tmp_path / "lits" / "a" / "output_fp_sample.npy").size == bench.DUMP_SAMPLE


def test_bench_dump_counts_share_the_budget_smallest_first():
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    assert bench._dump_counts([10, 5], [8, 8], [4, 8], budget=1000) == [8, 5]
    # 40 + 400 + 4000 bytes wanted, 1000 allowed: the arrays below their even share whole, the last one what is left
    assert bench._dump_counts([10, 100, 1000], [10 ** 6] * 3, [4, 4, 4], budget=1000) == [10, 100, 140]
    assert bench._dump_counts([10, 100, 1000], [10 ** 6] * 3, [4, 4, 4], budget=400) == [10, 45, 45]
