"""The fp64 restatement that tests/test_projection_gpu.py holds the projection kernels to (tests/projection_ref.py), anchored
to the oracle's own discretize, and the coverage of the inputs it is given.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.cpu_backend import OracleOps
from tests.projection_ref import (HAND_SCALES, SCREEN_BAND, host_state, projection_values, ref_levels, ref_project,
                                  screen_fallbacks, special_values, ulp_shift)

ALL_LEVELS = (2, 3, 4, 16, 128, 129, 255, 256, 257, 1024, 4096, 65536)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("levels", [2, 4, 16, 256])
@pytest.mark.parametrize("alpha", HAND_SCALES)
@pytest.mark.parametrize("dual_div", [1.0, 2.0, 1.25, 3.0])
def test_the_restatement_equals_the_oracle(levels, alpha, dual_div):
    n = 6000
    rng = np.random.default_rng(levels)
    v = projection_values(alpha, levels, n, seed=levels)
    wstar = (alpha * rng.standard_normal(n)).astype(np.float32)
    dual = (0.3 * alpha * rng.standard_normal(n)).astype(np.float32)
    level, G, du, Gq, _ = ref_project(v, wstar, dual, alpha, levels, dual_div)

    G_o, dual_o = torch.empty(n), torch.from_numpy(dual.copy())
    state = torch.from_numpy(host_state(alpha))
    OracleOps().admm_project_dual(torch.from_numpy(v), torch.from_numpy(wstar), state, levels, G_o, dual_o, dual_div)
    assert np.array_equal(_bits(G), _bits(G_o.numpy()))
    assert np.array_equal(_bits(du), _bits(dual_o.numpy()))
    # the level itself, from the oracle's index (its discretize before the affine map back)
    from oracle import effq_oracle as O
    idx = O.quant_index(torch.from_numpy(v).double() / alpha, levels, -1.0, 1.0).numpy()
    assert np.array_equal(level, idx)
    assert level.min() == 0 and level.max() == levels - 1
    # both encodings of the int8 numerators give back the level
    back = (Gq.astype(np.int64) + (levels - 1)) // 2 if levels <= 128 else Gq.astype(np.int64) + 128
    assert np.array_equal(back, level)


def test_the_next_right_hand_side_of_the_restatement():
    """Bm = (B0 + eta W0) + rho (G - dual'), the new dual: against the same sum in fp64 to fp32 rounding, and every element
    outside the weight columns left alone."""
    c2, nwrow, n, ldb = 6, 27, 28, 28
    rng = np.random.default_rng(3)
    alpha, levels = 0.73, 16
    v = projection_values(alpha, levels, c2 * nwrow, seed=1)
    v[~np.isfinite(v)] = alpha
    wstar, dual = (rng.standard_normal(c2 * nwrow).astype(np.float32) for _ in range(2))
    nxt = dict(B0=rng.standard_normal((c2, n)).astype(np.float32), W0=rng.standard_normal(c2 * nwrow).astype(np.float32),
               nwrow=nwrow, n=n, ldb=ldb, rho=37.3, eta=3.3, fill=np.float32(-7.25e33))
    _, G, du, _, Bm = ref_project(v, wstar, dual, alpha, levels, 2.0, nxt)
    want = (nxt["B0"][:, :nwrow].astype(np.float64) + np.float64(np.float32(3.3)) * nxt["W0"].reshape(c2, nwrow) +
            np.float64(np.float32(37.3)) * (G.astype(np.float64) - du).reshape(c2, nwrow))
    scale = np.abs(nxt["B0"]).max() + 3.3 * np.abs(nxt["W0"]).max() + 37.3 * (np.abs(G).max() + np.abs(du).max())
    assert np.abs(Bm[:, :nwrow] - want).max() <= 4 * 2.0 ** -24 * scale          # four fp32 roundings
    assert np.all(Bm[:, nwrow:] == nxt["fill"])
    # ... and it is the NEW dual that enters: the old one gives something else
    old = nxt["B0"][:, :nwrow] + np.float32(3.3) * nxt["W0"].reshape(c2, nwrow) + \
        np.float32(37.3) * (G - dual).reshape(c2, nwrow)
    assert not np.array_equal(_bits(old), _bits(Bm[:, :nwrow]))


def test_ulp_neighbours():
    x = np.array([1.0, -1.0, 0.0, -0.0, 1e-45, -1e-45], dtype=np.float32)
    up, down = ulp_shift(x, 1), ulp_shift(x, -1)
    assert np.array_equal(up, np.nextafter(x, np.float32(np.inf)))
    assert np.array_equal(down, np.nextafter(x, np.float32(-np.inf)))
    assert np.array_equal(ulp_shift(ulp_shift(x, 4), -4)[[0, 1, 4, 5]], x[[0, 1, 4, 5]])


@pytest.mark.parametrize("levels", ALL_LEVELS)
@pytest.mark.parametrize("alpha", HAND_SCALES)
def test_the_inputs_sit_on_every_boundary_and_inside_the_screens_band(levels, alpha):
    """What the generator promises: every level is hit, every rounding boundary has values on both sides within 4 ulp, at
    least 300 values lie inside the band in which the fp32 screen defers to the fp64 arithmetic (the band is 2e-4 of a
    level wide on either side of a boundary) and a few hundred just outside it, and the specials of the contract."""
    sp = special_values(alpha, levels, seed=5)
    assert np.array_equal(sp, special_values(alpha, levels, seed=5))           # deterministic by seed
    assert not np.isnan(sp).any()
    r, d = ref_levels(sp, alpha, levels)
    assert np.array_equal(np.unique(r), np.arange(levels))
    nb = levels - 1
    tight = sp[: 7 * nb].reshape(7, nb)                                        # the boundaries and their ulp neighbours
    rt = ref_levels(tight, alpha, levels)[0]
    j = np.arange(nb)
    # (the middle boundary of an even level count is v = 0, or ~1e-17 alpha as fp64 evaluates it: t + 1 is 1.0 for it and
    # for all its neighbours, (t + 1) / d the tie itself, and the level the even one; the spread values cover both sides)
    mid = np.abs(tight[0]) < 1e-9 * alpha
    assert np.count_nonzero(mid) <= 1
    assert np.all((rt.min(axis=0) == j) | mid) and np.all((rt.max(axis=0) == j + 1) | mid)
    u = (sp[np.isfinite(sp)].astype(np.float64) / alpha + 1.0) / d
    frac = np.abs(u - np.floor(u) - 0.5)
    inside = (frac < SCREEN_BAND) & (u > 0) & (u < levels - 1)
    assert SCREEN_BAND == pytest.approx(2e-4, rel=1e-3)
    assert np.count_nonzero(inside) >= 300
    assert np.count_nonzero((frac > SCREEN_BAND) & (frac < 3.1e-4)) >= 100
    if levels <= 256:                                                          # the screen as the kernels evaluate it
        assert screen_fallbacks(sp, alpha, levels) >= 300
    for want in (np.float32(alpha), np.float32(-alpha), np.float32(10 * alpha), np.float32(-10 * alpha),
                 np.float32(1e-40), np.float32(np.inf), np.float32(-np.inf)):
        assert np.any(sp == want)
    assert np.any((sp == 0) & ~np.signbit(sp)) and np.any((sp == 0) & np.signbit(sp))
    # a subset, the whole set, and the set with its fill
    assert projection_values(alpha, levels, 4, 1).shape == (4,)
    full = projection_values(alpha, levels, sp.size + 1000, 5)
    assert full.dtype == np.float32 and full.shape == (sp.size + 1000,) and np.isin(sp, full).all()


def test_struct_mirrors_have_the_layout_of_project_dual_h():
    from tests.projection_ref import ProjFused, ProjNext
    assert C.sizeof(ProjNext) == 48 and C.sizeof(ProjFused) == 112
    assert ProjNext.ldb.offset == 32 and ProjNext.rho.offset == 36 and ProjNext.eta.offset == 40
    assert ProjFused.d.offset == 40 and ProjFused.dual_div.offset == 48 and ProjFused.n4.offset == 56
    assert ProjFused.nx.offset == 64
