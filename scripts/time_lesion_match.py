"""effq_seg_lesion_match next to effq_seg_lesion_table on one BraTS-size case (3 classes, 155 x 240 x 240; diagnostic,
GPU): both called as the library is (tables of 2^18 rows and 2^18 pairs, no host read), alternating in one run, timed with
HIP events, median of REPS.  Two cases: blobs (smoothed seeded noise thresholded for the label, the same field shifted
and perturbed for the prediction: lesions that split, merge and drift) and the random logits of time_validation.py
against a label of density 0.1 (dust: as many pairs as the tables take).  Prints one JSON line; the time per launch is
read from a kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/time_lesion_match.py)."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from efficientq_amd import _lib
from efficientq_amd.hip_ops import get_ops

REPS = int(os.environ.get("REPS", "7"))
dev = "cuda:0"
shape = (155, 240, 240)
cap = capp = 1 << 18
ops = get_ops(dev)
thresh = ops.sigmoid_threshold()
ptr = lambda t: C.c_void_p(t.data_ptr())


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def smooth(x, k):
    return F.avg_pool3d(x[None], k, 1, k // 2)[0]


g = torch.Generator().manual_seed(0)
field = smooth(smooth(torch.randn(3, *shape, generator=g).to(dev), 9), 9)
field = field / field.std()
label_blobs = (field > 1.6).to(torch.uint8).contiguous()
noise = smooth(torch.randn(3, *shape, generator=g).to(dev), 5)
logits_blobs = (torch.roll(field, (1, 2, -1), (1, 2, 3)) + 0.5 * noise / noise.std() - 1.6).contiguous()
logits_dust = torch.randn(3, *shape, generator=g).to(dev)
label_dust = (torch.rand(3, *shape, generator=g) < 0.1).to(dev, torch.uint8)

counts = torch.empty(3, 4, dtype=torch.int64, device=dev)
nrows = torch.empty(6, dtype=torch.int64, device=dev)
rows = torch.empty(6, cap, 3, dtype=torch.int32, device=dev)
npairs = torch.empty(3, dtype=torch.int64, device=dev)
pairs = torch.empty(3, capp, 3, dtype=torch.int32, device=dev)
need_t = ops.lib.effq_cc_table_ws_bytes(6, *shape, cap)
need_m = ops.lib.effq_seg_lesion_match_ws_bytes(3, *shape, cap, capp)
ws = ops._workspace("cc", need_m)
fuse = _lib.SEG_FUSE[None]


def table(lg, lab):
    _lib.check(ops.lib.effq_seg_lesion_table(ptr(lg), ptr(lab), 3, *shape, _lib.SEG_SIGMOID, fuse, thresh,
                                             _lib.LESION_CONNECTIVITY, cap, ptr(counts), ptr(nrows), ptr(rows), ptr(ws),
                                             ws.numel(), ops.stream), "effq_seg_lesion_table")


def match(lg, lab):
    _lib.check(ops.lib.effq_seg_lesion_match(ptr(lg), ptr(lab), 3, *shape, _lib.SEG_SIGMOID, fuse, thresh,
                                             _lib.LESION_CONNECTIVITY, cap, capp, ptr(counts), ptr(nrows), ptr(rows),
                                             ptr(npairs), ptr(pairs), ptr(ws), ws.numel(), ops.stream),
               "effq_seg_lesion_match")


res = {"reps": REPS, "ws_table_MB": round(need_t / 1e6, 3), "ws_match_MB": round(need_m / 1e6, 3),
       "ws_match_default_KB": round((ops.lib.effq_seg_lesion_match_ws_bytes(3, *shape, _lib.LESION_TABLE_ROWS,
                                                                            _lib.LESION_PAIR_ROWS) -
                                     ops.lib.effq_cc_table_ws_bytes(6, *shape, _lib.LESION_TABLE_ROWS)) / 1e3, 1)}
for key, lg, lab in (("blobs", logits_blobs, label_blobs), ("dust", logits_dust, label_dust)):
    t1, m1 = timed(lambda: table(lg, lab)), timed(lambda: match(lg, lab))
    t2, m2 = timed(lambda: table(lg, lab)), timed(lambda: match(lg, lab))
    table(lg, lab)
    want = (counts.clone(), nrows.clone(), rows.clone())
    rows.fill_(0)
    match(lg, lab)
    n = nrows.tolist()
    same = torch.equal(counts, want[0]) and torch.equal(nrows, want[1]) and all(
        torch.equal(rows[q, :min(n[q], cap)], want[2][q, :min(n[q], cap)]) for q in range(6))
    res[key] = {"table_ms": [round(t1, 4), round(t2, 4)], "match_ms": [round(m1, 4), round(m2, 4)], "nrows": n,
                "npairs": npairs.tolist(), "shared_outputs_equal": bool(same)}
print(json.dumps(res))
