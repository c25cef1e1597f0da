// What the sweep (gptq.hip) and the coordinate-descent passes behind it (gptq_refine.hip) share: the block geometry, the
// cross-lane read of a double and the arithmetic of a committed weight.  No kernel lives here.
#pragma once
#include "common.h"

namespace effq {

typedef double gq_f64x4 __attribute__((ext_vector_type(4)));

constexpr int GQ_B = 64;          // block size of the factor, of the sweep and of the passes
constexpr int GQ_MAX_N = 32768;
constexpr int GQ_ROWS = 4;        // output rows (waves) per workgroup of k_gq_block and k_gr_block

__device__ __forceinline__ double gq_readlane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// f32(alpha) times the level value in the arithmetic that restores a stored weight, so that the round trip through the
// level ids gives these bits back: per row PTQConv._channel_weight (the value rounded from fp64), per tensor
// restore_fp_weight (id * f32(d) - 1 in fp32; the files that include this are compiled without contraction)
__device__ __forceinline__ float gq_weight_f32(double a, double idx, double d, int per_row) {
  const float bv = per_row ? (float)(idx * d - 1.0) : (float)idx * (float)d - 1.0f;
  return (float)a * bv;
}

}  // namespace effq
