"""--prep_denoise nlmM on the host: the switch, its columns, the host half of sigma, and the restatement itself."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from efficientq_amd import denoise as N, entrance, prep
from tests import prep_denoise_ref as R


@pytest.mark.parametrize("text, radius", [("nlm", 3), ("nlm1", 1), ("nlm2", 2), ("nlm3", 3), ("nlm4", 4), ("nlm5", 5),
                                          (None, None), ("nlm0", 0), ("nlm6", 0), ("nl", 0), ("n4", 0), ("NLM3x", 0)])
def test_the_grammar_of_the_switch_and_the_refusal_by_name(text, radius):
    if radius != 0:
        assert N.denoise_switch(SimpleNamespace(prep_denoise=text)) == radius
    else:
        with pytest.raises(prep.PrepError, match=f"--prep_denoise '{text}': nlm or nlmM"):
            N.denoise_switch(SimpleNamespace(prep_denoise=text))


@pytest.mark.parametrize("argv, named", [
    (["prep", "--task", "brats", "--src_list", "none.csv", "--data_dir", "o", "--prep_denoise", "nlm6"], "'nlm6': nlm or"),
    (["ptq", "--task", "brats", "--synthetic", "--prep_denoise", "nlm"], "ptq mission"),
    (["score", "--task", "lits", "--src_list", "c", "--pred_dir", ".", "--out_dir", "o", "--prep_denoise", "nlm"],
     "score mission"),
])
def test_the_missions_refuse_the_switch_by_name_before_a_file_is_read(argv, named):
    with pytest.raises(SystemExit) as e:
        entrance.main(argv)
    assert "--prep_denoise" in str(e.value) and named in str(e.value) and not os.path.exists("o")


def test_the_columns_stand_directly_before_the_bias_columns_and_only_with_the_switch():
    base = prep.PrepOptions("nonzero", None, None, (8, 8, 8), False)
    assert base.denoise is None and not set(prep.DENOISE_COLUMNS) & set(base.columns())
    assert not set(prep.DENOISE_COLUMNS) & set(base._replace(bias="n4", align="flair", interp="cubic").columns())
    head = base._replace(bias="n4", align="flair", interp="cubic", denoise=3).columns()
    at = head.index("denoise")
    assert head[at - 1] == "interp" and head[at:at + 8] == prep.DENOISE_COLUMNS + prep.BIAS_COLUMNS
    assert base._replace(denoise=2, align="flair").columns() == prep.DENOISE_COLUMNS + prep.ALIGN_COLUMNS


def test_the_host_half_of_the_noise_level():
    scale = 1.4826 * math.sqrt(6.0 / 7.0)
    assert N.sigma_of(5, 2.0, 7.0) == scale * 2.0                          # odd n: the middle one, k = 2, h - k = 0
    assert N.sigma_of(4, 2.0, 3.0) == scale * 2.5                          # even n: half way
    assert N.sigma_of(4, 0.1, 0.2) == scale * float(np.float32(0.1 + 0.5 * (0.2 - 0.1)))       # rounded to fp32
    assert R.sigma_of(np.float32([0, 3, 0, 1, 2, 0, 10])) == (N.sigma_of(4, 2.0, 3.0), 4) and N.H2 == R.H2


def test_the_restatement_on_a_constant_and_on_a_two_voxel_volume():
    c = np.full((4, 5, 6), 7.25, dtype=np.float32)
    assert not R.residual(c).any() and R.sigma_of(R.residual(c))[1] == 0
    y, spread, sumsq, count = R.nlm(c, "nonzero", 2, 1.0)
    assert np.array_equal(y, c) and not spread.any() and (sumsq, count) == (0.0, c.size)
    # two voxels a, b: every clamped patch of a holds 18 a and 9 b, of b 9 a and 18 b: d2 = 9 (a - b)^2 / 27
    v = np.float32([[[1.0, 4.0]]])
    d2, sigma = 9 * 9.0 / 27, 1.0
    w = math.exp(-max(d2 - 2 * sigma ** 2, 0.0) / sigma ** 2)
    y, spread, sumsq, count = R.nlm(v, "all", 1, sigma)
    assert np.allclose(y.ravel(), [(w * 4 + w * 1) / (2 * w), (w * 1 + w * 4) / (2 * w)], rtol=1e-15, atol=0)
    assert np.array_equal(spread.ravel(), [3.0, 3.0]) and count == 2 and math.isclose(sumsq, 2 * 1.5 ** 2, rel_tol=1e-14)
