// The geometry of a general affine gather that prep_align.hip and prep_register.hip share, so that a registration samples
// the moving volume exactly where the alignment that follows it does: the field of view of one axis and the trilinear
// footprint of one axis (the rule of prep.py's --prep_align, restated in include/effq_hip.h at effq_prep_align).
#pragma once
#include <math.h>
#include "common.h"

namespace effq {

// the field of view of one axis; false for a NaN
__device__ __forceinline__ bool in_fov(double s, unsigned n) { return s >= -0.5 && s < (double)n - 0.5; }

// the trilinear footprint of one axis at a coordinate inside the field of view
__device__ __forceinline__ void align_axis(double s, unsigned n, unsigned& i0, unsigned& i1, float& l0, float& l1) {
  const double top = (double)(n - 1);
  const double c = s < 0.0 ? 0.0 : (s > top ? top : s);
  const double fl = floor(c);
  i0 = (unsigned)fl;
  i1 = i0 + (i0 < n - 1 ? 1u : 0u);
  l1 = (float)(c - fl);
  l0 = 1.0f - l1;
}

}  // namespace effq
