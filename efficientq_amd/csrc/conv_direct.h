// Internal interface between conv3d.hip (the C-ABI entry conv3d_quant_calib_step) and conv3d_direct.hip.
#pragma once
#include "common.h"

namespace effq {

struct DirectParams {
  const float* x;       // NDHWC
  const float* G;       // reference weight layout [C2][C1][KD*KH*KW]
  const float* bias;
  const float* y;       // NDHWC target
  int N, C1, C2, D, H, W, OD, OH, OW, SD, SH, SW, PD, PH, PW;
  long long V;
  int ntiles;
  double* partials;
  unsigned int* ticket;
  double* sqerr;
};

// 0: not served; 1: 4-channel 3x3x3 conv onto 32 channels; 2: 1x1x1 conv onto <= 4 channels; 3: 1-channel 3x3x3 conv onto 32
int conv_direct_kind(const effq_geom* g);

// The launch conv_direct_launch makes for a kind: which kernel, its grid and the tiles it walks.  kernel: 0 none (the
// sizes are beyond the direct kernels' 32-bit indices: the tiled kernels serve the call), 1 k_conv3d_c4h<S>,
// 2 k_conv1_mfma, 3 k_conv3d_c1h<SD, SH, SW>, 4 k_conv3d_c4 (the 4-channel conv at every stride k_conv3d_c4h has no
// instance for).  ntiles: 4 x 4 x 8 output tiles (td x th x tw per volume) for kernels 1 and 3, 32-voxel wave tiles for 4,
// 16-voxel wave tiles for 2.
struct DirectLaunch {
  int kernel;
  unsigned grid;
  int td, th, tw, ntiles;
};
DirectLaunch conv_direct_plan(int kind, const DirectParams& p, size_t max_blocks);
int conv_direct_launch(int kind, DirectParams& p, size_t max_blocks, hipStream_t st);

}  // namespace effq
