"""predict --crf on the host: the switches and their refusals in all four missions, the radii, and the restatement itself."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from efficientq_amd import config as Cf, crf, entrance
from tests import seg_crf_ref as R

PREDICT = ["predict", "--task", "lits", "--src_list", "none.csv", "--out_dir", "o", "--pretrain", "none.pkl", "--qconv", "conv"]
OTHERS = {"ptq": ["ptq", "--task", "brats", "--synthetic"],
          "prep": ["prep", "--task", "brats", "--src_list", "none.csv", "--data_dir", "o"],
          "score": ["score", "--task", "lits", "--src_list", "c", "--pred_dir", ".", "--out_dir", "o"]}
SWITCHES = {"crf": [], "crf_w": ["4,1"], "crf_theta": ["3,0.5,1"], "crf_iters": ["5"]}


def parse(*argv):
    return Cf.build_parser().parse_args(["predict"] + list(argv))


def test_the_switches_their_defaults_and_the_yaml_keys(tmp_path):
    assert crf.crf_switches(parse()) is None
    assert crf.crf_switches(parse("--crf")) == crf.DEFAULTS == (4.0, 1.0, 3.0, 0.5, 1.0, 5)
    got = crf.crf_switches(parse("--crf", "--crf_w", "2.5,0", "--crf_theta", "4,0.25,1.5", "--crf_iters", "20"))
    assert got == (2.5, 0.0, 4.0, 0.25, 1.5, 20) and crf.column_text(got) == "2.5 0 4 0.25 1.5 20"
    cfg = tmp_path / "c.yaml"
    cfg.write_text("crf: true\ncrf_w: [3, 2]\ncrf_theta: '2,1,1'\ncrf_iters: 3\n")
    assert crf.crf_switches(Cf.merge_config(str(cfg), parse())) == (3.0, 2.0, 2.0, 1.0, 1.0, 3)
    assert "not tuned" in crf.said(crf.DEFAULTS) and "score" in crf.said(got)


@pytest.mark.parametrize("switch, value", [
    ("crf_w", "4"), ("crf_w", "4,1,1"), ("crf_w", "-1,1"), ("crf_w", "60,4.5"), ("crf_w", "a,1"), ("crf_w", "nan,1"),
    ("crf_theta", "3,0.5"), ("crf_theta", "3,0,1"), ("crf_theta", "3,0.5,-1"), ("crf_theta", "3,inf,1"),
    ("crf_theta", "3,0.5,1e-19"), ("crf_theta", "3,1e19,1"),
    ("crf_iters", "0"), ("crf_iters", "21"), ("crf_iters", "2.5"), ("crf_iters", "x")])
def test_a_malformed_value_is_refused_by_name_before_a_file_is_read(switch, value, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        entrance.main(PREDICT + ["--crf", f"--{switch}", value])
    assert str(e.value).startswith(f"--{switch} '{value}'") and not os.path.exists("o")


@pytest.mark.parametrize("switch", ["crf_w", "crf_theta", "crf_iters"])
def test_a_qualifier_without_the_switch_is_refused_by_name(switch, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit, match=f"--{switch} qualifies --crf"):
        entrance.main(PREDICT + [f"--{switch}"] + SWITCHES[switch])
    assert not os.path.exists("o")


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("mission", list(OTHERS))
def test_the_other_missions_refuse_all_four_by_name(mission, switch, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        entrance.main(OTHERS[mission] + [f"--{switch}"] + SWITCHES[switch])
    assert str(e.value).startswith(f"--{switch} ") and f"the {mission} mission" in str(e.value) and not os.path.exists("o")


@pytest.mark.parametrize("spacing, want", [((1, 1, 1), (3, 3, 3)), ((2.5, 0.8, 0.8), (2, 3, 3)), ((7, 1, 1), (0, 3, 3))])
def test_the_radii_from_the_spacing(spacing, want):
    assert crf.radii(spacing, crf.DEFAULTS) == want == R.radii(spacing, 3.0, 1.0)


def test_a_grid_with_no_linked_axis_is_refused_naming_subject_and_spacing():
    from efficientq_amd.prep import PrepError
    with pytest.raises(PrepError, match="subject s7: --crf: at the working spacing 7 8 9 mm"):
        crf.refine(SimpleNamespace(), "s7", None, None, (7, 8, 9), "softmax", crf.DEFAULTS)


def test_the_restatement_without_weights_and_on_a_constant_image():
    g = np.random.default_rng(0)
    v = (4 * g.standard_normal((3, 5, 6, 7))).astype(np.float32)
    x = g.standard_normal((2, 5, 6, 7)).astype(np.float32)
    for mode in ("softmax", "sigmoid"):
        h, changed, ok = R.crf(v, x, (1, 1, 1), mode, 0.0, 0.0, 3.0, 0.5, 1.0, 5)
        assert np.array_equal(h, v.astype(np.float64)) and changed == 0 and ok.all()
    # a constant image, every voxel sure of class 1: an interior voxel receives exactly w_a + w_s for that class
    v = np.zeros((2, 9, 9, 9), dtype=np.float32)
    v[1] = 1000.0
    h, _, _ = R.crf(v, np.full((1, 9, 9, 9), 0.5, dtype=np.float32), (1, 1, 1), "softmax", 4.0, 1.0, 3.0, 0.5, 1.0, 1)
    assert abs(h[1, 4, 4, 4] - 1005.0) < 1e-12 and h[0, 4, 4, 4] == 0.0 and h[1, 0, 4, 4] < 1004.0
    h, _, _ = R.crf(v, np.full((1, 9, 9, 9), 0.5, dtype=np.float32), (1, 1, 1), "sigmoid", 4.0, 1.0, 3.0, 0.5, 1.0, 1)
    assert abs(h[1, 4, 4, 4] - 1005.0) < 1e-12 and h[0, 4, 4, 4] == 0.0              # 2 sigmoid(0) - 1 = 0
