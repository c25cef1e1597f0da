"""--prep_bias n4 on the host: the switch, the sharpening, the sample rule, and the missions on a stand-in."""
import csv
import os

import numpy as np
import pytest

from efficientq_amd import bias as B, entrance, predict, prep
from tests import prep_bias_backend as K, prep_bias_ref as R
from tests import test_prep_align_cpu as H
from tests.test_prep_cpu import prep_args, write_list, write_subjects, written


class BiasOps(K.BiasMixin, H.AlignOps):
    """The stand-in for the device with the calls of the correction."""


@pytest.mark.parametrize("argv, named", [
    (["prep", "--task", "brats", "--src_list", "none.csv", "--data_dir", "o", "--prep_bias", "n3"], "--prep_bias 'n3': n4"),
    (["predict", "--task", "brats", "--src_list", "none.csv", "--out_dir", "o", "--resume", __file__, "--prep_bias", "N5"],
     "--prep_bias 'N5': n4"),          # the snapshot only has to exist: the switch is refused before it is opened
    (["ptq", "--task", "brats", "--synthetic", "--prep_bias", "n4"], "ptq mission"),
    (["score", "--task", "lits", "--src_list", "c", "--pred_dir", ".", "--out_dir", "o", "--prep_bias", "n4"],
     "score mission"),
])
def test_the_switch_is_refused_by_name_before_a_file_is_read(argv, named):
    with pytest.raises(SystemExit) as e:
        entrance.main(argv)
    assert "--prep_bias" in str(e.value) and named in str(e.value) and not os.path.exists("o")


def test_sharpening_of_a_two_peak_histogram_against_the_restatement():
    lo, hi = -0.4, 0.9
    centre = lo + np.arange(R.BINS) * (hi - lo) / (R.BINS - 1)
    h = 4000 * np.exp(-((centre + 0.1) / 0.08) ** 2) + 2500 * np.exp(-((centre - 0.5) / 0.12) ** 2)
    got, want = B.sharpen(h, lo, hi), R.sharpen(h, lo, hi)
    assert np.allclose(got, want, rtol=0, atol=1e-10) and np.ptp(got) > 0.5


@pytest.mark.parametrize("extent, want", [(240, (4, 2, 60)), (32, (4, 2, 8)), (33, (4, 2, 8)), (31, (4, 2, 8)), (29, (1, 0, 29)), (3, (1, 0, 3))])
def test_sample_rule(extent, want):
    s, o = B.sample_rule(extent)
    index = np.arange(o, extent, s)
    assert (s, o, len(index)) == want and np.array_equal(index, R.samples(extent))


def test_missions_write_the_columns_at_their_place_and_only_with_the_switch(tmp_path, capsys):
    root = str(tmp_path)
    rows, _ = write_subjects(root, ["b1"], [5])
    lst = write_list(tmp_path / "cases.csv", rows)
    kw = dict(src_list=lst, prep_min_size="8,8,8")
    prep.run(prep_args(data_dir=os.path.join(root, "plain"), **kw), ops=H.AlignOps())
    prep.run(prep_args(data_dir=os.path.join(root, "again"), **kw), ops=BiasOps())
    for name in written(os.path.join(root, "plain")):          # without the switch nothing changes
        one, two = (open(os.path.join(root, d, name), "rb").read() for d in ("plain", "again"))
        assert one == two, name
    capsys.readouterr()
    prep.run(prep_args(data_dir=os.path.join(root, "n4"), prep_bias="n4", prep_align="flair", **kw), ops=BiasOps())
    said = capsys.readouterr().out
    table = list(csv.DictReader(open(os.path.join(root, "n4", prep.PREP_CSV))))
    head = list(table[0])
    assert head[head.index("bias"):head.index("bias") + 6] == prep.BIAS_COLUMNS + prep.ALIGN_COLUMNS
    row = table[0]
    iters = [[int(n) for n in part.split()] for part in row["bias_iters"].split(";")]
    assert row["bias"] == "n4" and len(iters) == 4 and all(len(i) == 4 and 1 <= min(i) and max(i) <= 50 for i in iters)
    fields = [[float(v) for v in part.split()] for part in row["bias_field"].split(";")]
    assert len(row["bias_cv"].split(";")) == 4 and all(0 < lo <= hi < np.inf for lo, hi in fields)
    assert f", bias flair {fields[0][0]:.2f}-{fields[0][1]:.2f} ({' '.join(map(str, iters[0]))} it)" in said
    assert not np.array_equal(np.load(os.path.join(root, "n4", "flair", "b1.npy")),
                              np.load(os.path.join(root, "plain", "flair", "b1.npy")))
    kw = dict(src_list=write_list(tmp_path / "p.csv", [rows[0][:5]], head=("subject",) + H.MODS),
              out_dir=os.path.join(root, "seg"), patch_size="8,8,8", prep_min_size="8,8,8")
    got = predict.run(H.predict_args(prep_bias="n4", prep_align="flair", **kw), ops=BiasOps(), model=H.FourNet(),
                      window_batch=3)
    head = list(csv.reader(open(os.path.join(root, "seg", predict.PREDICT_CSV))))[0]
    assert head == predict.CSV_HEADER + prep.BIAS_COLUMNS + prep.ALIGN_COLUMNS and got[0]["bias_iters"] == row["bias_iters"]

