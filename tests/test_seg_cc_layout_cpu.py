"""The layout of the connected-component sources: the labelling (seg_cc.hip), the lesion table (seg_cc_table.hip) and the
rules of --post (label_post.hip) share seg_cc.h, and the wave sums of the library live in common.h alone.  Text only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "efficientq_amd", "csrc")

ENTRY_POINTS = {
    "seg_cc.hip": ("effq_cc_ws_bytes", "effq_cc_label", "effq_seg_lesions"),
    "seg_cc_table.hip": ("effq_cc_table_ws_bytes", "effq_cc_table", "effq_seg_lesion_table"),
    "label_post.hip": ("effq_label_clean_ws_bytes", "effq_label_clean", "effq_label_post_ws_bytes", "effq_label_post"),
}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _sources(pattern):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, pattern)))


def test_the_makefile_builds_the_three_files_and_tracks_the_header():
    mk = _read("Makefile")
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    for name in ENTRY_POINTS:
        assert srcs.count(name) == 1, name
    rule = re.search(r"^%\.o:(.*)$", mk, re.M).group(1).split()
    assert "seg_cc.h" in rule


def test_every_entry_point_is_defined_once_and_in_its_file():
    texts = {name: _read(name) for name in _sources("*.hip")}
    for home, names in ENTRY_POINTS.items():
        for fn in names:
            # a definition: return type, name, argument list, opening brace (a call or a declaration has none)
            pat = re.compile(rf"^(?:int|size_t) {fn}\s*\([^;{{]*\)\s*\{{", re.M)
            owners = [name for name, text in texts.items() for _ in pat.findall(text)]
            assert owners == [home], (fn, owners)


def test_only_label_post_pulls_in_the_distance_transform():
    assert '#include "seg_surf.h"' in _read("label_post.hip")
    for name in ("seg_cc.hip", "seg_cc_table.hip", "seg_cc.h"):
        assert "seg_surf.h" not in _read(name), name
    for name in ENTRY_POINTS:
        assert '#include "seg_cc.h"' in _read(name), name


def test_the_shared_header_holds_no_kernel():
    hdr = _read("seg_cc.h")
    assert "__global__" not in hdr
    assert re.search(r"^int cc_run\s*\(", hdr, re.M) and "static int cc_run" not in _read("seg_cc.hip")


def test_wave_sums_are_defined_in_common_h_alone():
    define = re.compile(r"^[ \t]*(?:__device__|__host__|static|inline|template)[^;\n]*?\b(wave_sum\w*)\s*\([^;{]*\)\s*\{", re.M)
    assert {"wave_sum", "wave_sum_all"} <= set(define.findall(_read("common.h")))
    for name in _sources("*.hip") + _sources("*.h"):
        if name != "common.h":
            assert define.findall(_read(name)) == [], name
