// The per-voxel decisions of the validation kernels: which classes a voxel is predicted as and labelled as.  One
// definition for the tallies, the label maps (seg_eval.hip), the lesion counts (seg_cc.hip) and the agreement of two
// networks (seg_agree.hip), so that they cannot disagree about a voxel.
#pragma once
#include "common.h"

namespace effq {

// the predicted classes of one voxel from its C logits: bit c for class c (needs no label: seg_agree.hip decides both
// networks' voxels with it)
template <int MODE, int C>
__device__ __forceinline__ uint32_t predict(const float* v, int fuse, float thresh) {
  uint32_t pred = 0;
  if constexpr (MODE == EFFQ_SEG_ARGMAX) {
    // torch.max over the channels: the first maximum wins, NaN counts as the largest value
    int best = 0;
    float bv = v[0];
#pragma unroll
    for (int c = 1; c < C; ++c) {
      const float x = v[c];
      if (x > bv || (x != x && bv == bv)) {
        bv = x;
        best = c;
      }
    }
    pred = 1u << best;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) pred |= (v[c] >= thresh ? 1u : 0u) << c;
    if (fuse == EFFQ_SEG_FUSE_AGG) {        // p[i] = any(p[i:])
      uint32_t f = 0, any = 0;
#pragma unroll
      for (int c = C - 1; c >= 0; --c) {
        any |= (pred >> c) & 1u;
        f |= any << c;
      }
      pred = f;
    } else if (fuse == EFFQ_SEG_FUSE_CON) { // p[i] = all(p[:i+1])
      uint32_t f = 0, all = 1;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        all &= (pred >> c) & 1u;
        f |= all << c;
      }
      pred = f;
    }
  }
  return pred;
}

// the label of one voxel from its predicted classes, for the label maps on the working grid (seg_eval.hip) and on the
// source grid (seg_source.hip)
template <int RULE, int C>
__device__ __forceinline__ uint32_t label_of(uint32_t pred) {
  if constexpr (RULE == EFFQ_SEG_LABEL_ARGMAX) {
    return 31 - __builtin_clz(pred);                  // pred = 1 << winning class
  } else if constexpr (RULE == EFFQ_SEG_LABEL_BRATS) {
    // misc.merge_label_brats, later assignments winning: WT -> 1, WT and not TC -> 2, ET -> 4
    uint32_t l = 0;
    if (pred & 1u) l = 1;
    if ((pred & 3u) == 1u) l = 2;
    if (pred & 4u) l = 4;
    return l;
  } else {                                            // RANK: i + 1 of the highest set channel, 0 when none
    return pred ? 32 - __builtin_clz(pred) : 0u;
  }
}

// the decisions of one voxel: pred / gt bit c for class c
template <int MODE, int C>
__device__ __forceinline__ void decide(const float* v, const uint8_t* lab, int fuse, float thresh, uint32_t& pred,
                                       uint32_t& gt) {
  pred = predict<MODE, C>(v, fuse, thresh);
  gt = 0;
  if constexpr (MODE == EFFQ_SEG_ARGMAX) {
    const int l = lab[0];
    gt = l < C ? (1u << l) : 0u;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) gt |= (lab[c] != 0 ? 1u : 0u) << c;
  }
}

}  // namespace effq
