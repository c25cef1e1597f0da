// What the two kernels that read stitched logits at the voxels of a SOURCE grid share (seg_source.hip: one label per
// voxel; seg_prob.hip: probabilities and an uncertainty per voxel): the per-axis inverse map with its inside rule, the
// eight-corner fp32 blend, the row-item launch shape, the 4-byte store and the argument checks.  One definition, so that
// the label map and the probability maps of a subject cannot disagree about where a voxel lies or what its interpolated
// logits are.  The rule itself is stated at the head of seg_source.hip and in DESIGN section 15.
#pragma once
#include "common.h"

namespace effq {

constexpr int SRC_THREADS = 256;
constexpr int SRC_MAX_BLOCKS = 4096;

struct __attribute__((packed, aligned(1))) SByte4 { uint8_t x, y, z, w; };

struct SrcAxis {
  unsigned i0, i1;
  float l0, l1;
  bool inside;
};

__device__ __forceinline__ SrcAxis src_axis(unsigned s, double f, int G, int pmin, int g) {
  SrcAxis a;
  const double t = ((double)s + 0.5) / f;
  double n = floor(t);
  const double last = (double)(G - 1);
  n = n > last ? last : n;
  a.inside = n >= (double)pmin && n < (double)(pmin + g);
  double q = t - 0.5 - (double)pmin;
  const double top = (double)(g - 1);
  q = q < 0.0 ? 0.0 : (q > top ? top : q);
  const double fl = floor(q);
  a.i0 = (unsigned)fl;
  a.i1 = a.i0 + (a.i0 < (unsigned)(g - 1) ? 1u : 0u);
  a.l1 = (float)(q - fl);
  a.l0 = 1.0f - a.l1;
  return a;
}

// One channel's logit at one source voxel from its eight corners.  r00, r01, r10, r11: channel 0's rows (i0d, i0h),
// (i0d, i1h), (i1d, i0h), (i1d, i1h) of the box; o: the channel's plane offset.  The order of k_prep_resample_linear:
// l0d (l0h (l0w v000 + l1w v001) + l1h (...)) + l1d (...), fp32, nothing fused.
__device__ __forceinline__ float src_blend(const float* r00, const float* r01, const float* r10, const float* r11,
                                           unsigned o, const SrcAxis& ad, const SrcAxis& ah, const SrcAxis& aw) {
  const float a = ad.l0 * (ah.l0 * (aw.l0 * r00[o + aw.i0] + aw.l1 * r00[o + aw.i1]) +
                           ah.l1 * (aw.l0 * r01[o + aw.i0] + aw.l1 * r01[o + aw.i1]));
  const float b = ad.l1 * (ah.l0 * (aw.l0 * r10[o + aw.i0] + aw.l1 * r10[o + aw.i1]) +
                           ah.l1 * (aw.l0 * r11[o + aw.i0] + aw.l1 * r11[o + aw.i1]));
  return a + b;
}

// The four bytes of one row item, w0 .. w0 + 3 of a row of SW: one 4-byte store (aligned when al4: every group of four
// of the plane lies on a 4-B boundary), single bytes for the tail of a row whose SW is no multiple of 4.
__device__ __forceinline__ void src_store4(uint8_t* dst, const uint8_t* b, unsigned w0, unsigned SW, int al4) {
  if (w0 + 4 <= SW) {
    if (al4) {
      *reinterpret_cast<uchar4*>(dst) = make_uchar4(b[0], b[1], b[2], b[3]);
    } else {
      SByte4 o;
      o.x = b[0]; o.y = b[1]; o.z = b[2]; o.w = b[3];
      *reinterpret_cast<SByte4*>(dst) = o;
    }
  } else {
    for (unsigned u = 0; w0 + u < SW; ++u) dst[u] = b[u];
  }
}

// the checks of prep_fits (prep.hip)
static inline bool source_fits(long long N, long long D, long long H, long long W) {
  return N > 0 && D > 0 && H > 0 && W > 0 && D <= 32767 && H <= 32767 && W <= 32767 && N * D * H * W < (1ll << 31);
}

// the workgroups of a launch over the row items of a source grid: one thread per item, SRC_MAX_BLOCKS at most (the
// kernels stride over the rest)
static inline unsigned source_blocks(const int* source) {
  const size_t items = (size_t)source[0] * source[1] * ((source[2] + 3) / 4);
  size_t nb = (items + SRC_THREADS - 1) / SRC_THREADS;
  nb = nb < 1 ? 1 : (nb > (size_t)SRC_MAX_BLOCKS ? (size_t)SRC_MAX_BLOCKS : nb);
  return (unsigned)nb;
}

}  // namespace effq
