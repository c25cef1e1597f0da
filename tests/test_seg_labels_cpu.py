"""The label-map kernel's host side (no GPU): its C-ABI row and rule codes against include/effq_hip.h, and the rule
validate_seg picks for each label form."""
import os
import re

import pytest

from efficientq_amd import _lib, evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seg_labels_symbol_and_rules_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "effq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint effq_seg_labels\s*\(", hdr)
    assert "effq_seg_labels" in _lib.SIGNATURES
    for name, code in _lib.SEG_LABEL_RULES.items():
        m = re.search(rf"#define EFFQ_SEG_LABEL_{name.upper()} (\d+)", hdr)
        assert m and int(m.group(1)) == code, name


def test_validation_map_rule_follows_the_label_form():
    assert E.label_rule(False) == "argmax"
    assert E.label_rule(False, "brats", "brats") == "argmax"
    assert E.label_rule(True, "brats", "brats") == "brats"
    assert E.label_rule(True, "lits", "lits") == "planes"
    assert E.label_rule(True, None, "brats") == "brats"
    assert E.label_rule(True, None, "lits") == "planes"
    with pytest.raises(RuntimeError):
        E.label_rule(True, "kits", "lits")
