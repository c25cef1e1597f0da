// The last step of the `predict` mission (predict.py): the stitched logits of one subject, which live on the cropped box
// pmin : pmin + g of the working grid G, turned into one label per voxel of the SOURCE grid (SD, SH, SW) the scan came
// on.  The working grid came from the source grid through effq_prep_resample with the factors f = target spacing /
// source spacing (f = 1 without --prep_spacing): working voxel o lies at source coordinate (o + 0.5) f - 0.5 (lin_axis
// of prep.hip).  Per axis, for source index s, in fp64:
//   t = (s + 0.5) / f                        the working-grid coordinate of the voxel's centre, in voxel edges
//   n = min(floor(t), G - 1)                 the working voxel the centre falls in: inside iff pmin <= n < pmin + g
//   q = clamp(t - 0.5 - pmin, 0, g - 1)      the interpolation point in the box, i0 = floor(q), i1 = min(i0 + 1, g - 1),
//                                            l1 = float(q - i0), l0 = 1.0f - l1
// A voxel outside the box on any axis gets label 0.  Inside, each of the C logits is interpolated trilinearly in fp32 in
// the nesting order of k_prep_resample_linear, nothing fused, and the C values are decided by predict<MODE, C> and
// mapped by label_of<RULE, C> (seg_decide.h): the decisions and the labels of effq_seg_labels.  The logits are
// interpolated, not the probabilities: the sigmoid is monotone, so `v >= thresh` decides the same, and the argmax needs
// no exponential.
//
// Shaped like the row-wise kernels of prep.hip: a row item is four consecutive w of one source row, one thread each.  The
// d and h axes are worked out once per row item - shared by its four voxels, not by the row: the SW / 4 items of a row
// each repeat the two fp64 divisions - the w axis per voxel, and the four labels leave in one 4-byte store.  Eight corner
// reads per channel and voxel, neighbours in w share lines, the d and h corners come back from L2; measured, the pass runs
// at about a tenth of the HBM rate: the gather and the per-voxel work set its time, not the bytes.  No atomics, no reductions: equal inputs
// give equal bits.  Every index is 32-bit: the voxel counts are checked to lie below 2^31.
// src_axis, the eight-corner blend, the store and the checks live in seg_source.h, shared with seg_prob.hip.
#include "common.h"
#include "seg_decide.h"
#include "seg_source.h"

namespace effq {

struct SourceParams {
  const float* logits;      // (C, gd, gh, gw)
  uint8_t* out;             // (SD, SH, SW)
  unsigned SD, SH, SW;      // source grid
  int G[3], pmin[3], g[3];  // working grid, low corner and extent of the box
  double f[3];
  int fuse, al4;            // al4: every group of four lies on a 4-B boundary
  float thresh;
};

template <int RULE, int C>
__global__ __launch_bounds__(SRC_THREADS) void k_seg_labels_source(SourceParams p) {
  constexpr int MODE = RULE == EFFQ_SEG_LABEL_ARGMAX ? EFFQ_SEG_ARGMAX : EFFQ_SEG_SIGMOID;
  const unsigned gw4 = (p.SW + 3) / 4, total = p.SD * p.SH * gw4;
  const unsigned gh = (unsigned)p.g[1], gw = (unsigned)p.g[2];
  const unsigned plane = (unsigned)p.g[0] * gh * gw;
  for (unsigned e = blockIdx.x * SRC_THREADS + threadIdx.x; e < total; e += gridDim.x * SRC_THREADS) {
    const unsigned row = e / gw4, w0 = (e - row * gw4) * 4;
    const unsigned d = row / p.SH, h = row - d * p.SH;
    const SrcAxis ad = src_axis(d, p.f[0], p.G[0], p.pmin[0], p.g[0]);
    const SrcAxis ah = src_axis(h, p.f[1], p.G[1], p.pmin[1], p.g[1]);
    uint8_t lab[4] = {0, 0, 0, 0};
    if (ad.inside && ah.inside) {
      const float* r00 = p.logits + (ad.i0 * gh + ah.i0) * gw;
      const float* r01 = p.logits + (ad.i0 * gh + ah.i1) * gw;
      const float* r10 = p.logits + (ad.i1 * gh + ah.i0) * gw;
      const float* r11 = p.logits + (ad.i1 * gh + ah.i1) * gw;
#pragma unroll
      for (unsigned u = 0; u < 4; ++u) {
        const unsigned w = min(w0 + u, p.SW - 1);
        const SrcAxis aw = src_axis(w, p.f[2], p.G[2], p.pmin[2], p.g[2]);
        if (!aw.inside) continue;
        float v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          v[c] = src_blend(r00, r01, r10, r11, (unsigned)c * plane, ad, ah, aw);   // seg_source.h: the fp32 nesting order
        }
        lab[u] = (uint8_t)label_of<RULE, C>(predict<MODE, C>(v, p.fuse, p.thresh));
      }
    }
    src_store4(p.out + (size_t)row * p.SW + w0, lab, w0, p.SW, p.al4);
  }
}

template <int C>
static void launch_source(int rule, dim3 g, hipStream_t st, const SourceParams& p) {
  const dim3 t(SRC_THREADS);
  switch (rule) {
    case EFFQ_SEG_LABEL_ARGMAX: hipLaunchKernelGGL((k_seg_labels_source<EFFQ_SEG_LABEL_ARGMAX, C>), g, t, 0, st, p); break;
    case EFFQ_SEG_LABEL_BRATS: hipLaunchKernelGGL((k_seg_labels_source<EFFQ_SEG_LABEL_BRATS, C>), g, t, 0, st, p); break;
    default: hipLaunchKernelGGL((k_seg_labels_source<EFFQ_SEG_LABEL_RANK, C>), g, t, 0, st, p); break;
  }
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_seg_labels_source(const float* logits, int C, const int* box, const int* pmin, const int* grid,
                           const double* factors, const int* source, int rule, int fuse, float thresh, uint8_t* out,
                           void* stream) {
  EFFQ_CHECK_ARG(logits && box && pmin && grid && factors && source && out);
  EFFQ_CHECK_ARG(C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(rule == EFFQ_SEG_LABEL_ARGMAX || rule == EFFQ_SEG_LABEL_BRATS || rule == EFFQ_SEG_LABEL_RANK);
  EFFQ_CHECK_ARG(fuse == EFFQ_SEG_FUSE_NONE || fuse == EFFQ_SEG_FUSE_AGG || fuse == EFFQ_SEG_FUSE_CON);
  EFFQ_CHECK_ARG(rule != EFFQ_SEG_LABEL_ARGMAX || fuse == EFFQ_SEG_FUSE_NONE);
  EFFQ_CHECK_ARG(rule != EFFQ_SEG_LABEL_BRATS || C >= 3);
  EFFQ_CHECK_ARG(source_fits(1, source[0], source[1], source[2]));
  EFFQ_CHECK_ARG(source_fits(1, grid[0], grid[1], grid[2]));
  EFFQ_CHECK_ARG(source_fits(C, box[0], box[1], box[2]));
  for (int a = 0; a < 3; ++a) {
    EFFQ_CHECK_ARG(0 <= pmin[a] && pmin[a] <= grid[a] - box[a]);
    EFFQ_CHECK_ARG(factors[a] > 0.0 && factors[a] <= 1e6);          // false for a NaN
  }
  EFFQ_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 3) == 0);
  SourceParams p;
  p.logits = logits; p.out = out;
  p.SD = source[0]; p.SH = source[1]; p.SW = source[2];
  for (int a = 0; a < 3; ++a) { p.G[a] = grid[a]; p.pmin[a] = pmin[a]; p.g[a] = box[a]; p.f[a] = factors[a]; }
  p.fuse = fuse; p.thresh = thresh;
  p.al4 = source[2] % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  const dim3 g(source_blocks(source));
  const hipStream_t st = as_stream(stream);
  switch (C) {
    case 1: launch_source<1>(rule, g, st, p); break;
    case 2: launch_source<2>(rule, g, st, p); break;
    case 3: launch_source<3>(rule, g, st, p); break;
    case 4: launch_source<4>(rule, g, st, p); break;
    case 5: launch_source<5>(rule, g, st, p); break;
    case 6: launch_source<6>(rule, g, st, p); break;
    case 7: launch_source<7>(rule, g, st, p); break;
    default: launch_source<8>(rule, g, st, p); break;
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
