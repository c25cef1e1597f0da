// Scoring a finished label map against a label map (the `score` mission, score.py): the lesion counts of two uint8
// maps.  The contract is in include/effq_hip.h, the launch list in DESIGN section 26.  Phases of a call, in launch order:
//   bits     k_label_bits (label_bits.h): the 16 decision bits per voxel of seg_masks.h from the two maps and the table
//   label .. final   cc_run of seg_cc.hip on those bits, as effq_seg_lesions runs it
// The surface distances of the same bits (effq_label_surface_mm) live beside the reduce they share, in seg_surface_mm.hip.
#include "common.h"
#include "label_bits.h"
#include "seg_cc.h"

using namespace effq;

extern "C" {

int effq_label_lesions(const uint8_t* pred, const uint8_t* truth, int C, int D, int H, int W, const uint16_t* lut,
                       int connectivity, long long* counts, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(pred && truth && lut && counts && ws && C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(cc_dims_ok(2 * C, D, H, W));
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  EFFQ_CHECK_ARG(label_lut_ok(lut, C));
  const int P = 2 * C;
  const size_t S = (size_t)D * H * W;
  const CcWs s = cc_ws(ws, P, S);
  EFFQ_CHECK_WS(ws_bytes, s.bytes);
  const hipStream_t st = as_stream(stream);
  const int rc = label_decision_bits(pred, truth, lut, S, s.bits, st);
  if (rc != EFFQ_OK) return rc;
  return cc_run(cc_src_bits(s.bits, C), P, D, H, W, connectivity, s.labels, s.flags, C, s.partial, counts, st);
}

}  // extern "C"
