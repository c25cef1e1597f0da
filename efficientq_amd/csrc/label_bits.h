// The decision bits of one case from two uint8 label maps instead of logits and a label: the front of the entry points
// that score a finished map (effq_label_lesions in label_score.hip, effq_label_surface_mm in seg_surface_mm.hip).  The
// bits are those of seg_masks.h, pred | gt << 8, with the class bits of a value taken from a 256-entry table as
// effq_label_tallies takes them.  Internal linkage: each of the two files has its own k_label_bits.
#pragma once
#include "common.h"
#include "seg_masks.h"

namespace effq {

struct LabelBitsLut {
  uint16_t v[256];
};

// every entry of the table of C classes names classes below C only
static inline bool label_lut_ok(const uint16_t* lut, int C) {
  for (int v = 0; v < 256; ++v)
    if (lut[v] >> C) return false;
  return true;
}

// bits[v] = (lut[pred[v]] & 0xff) | (lut[truth[v]] & 0xff) << 8.  The table is staged in LDS once per workgroup (a
// per-lane index into a kernel argument would go to scratch).  VEC 4: one 4-B load per map and one 8-B store per thread;
// the last S % 4 voxels are written one by one by the first threads of the grid.
template <int VEC>
static __global__ __launch_bounds__(CC_THREADS) void k_label_bits(const uint8_t* __restrict__ pred,
                                                                  const uint8_t* __restrict__ truth,
                                                                  uint16_t* __restrict__ bits, long long S,
                                                                  LabelBitsLut lut) {
  __shared__ uint16_t s_lut[256];
  for (int k = threadIdx.x; k < 256; k += CC_THREADS) s_lut[k] = lut.v[k] & 0xffu;
  __syncthreads();
  auto one = [&](uint8_t p, uint8_t t) { return (uint16_t)(s_lut[p] | (s_lut[t] << 8)); };
  const long long groups = S / VEC;
  const long long tid = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  for (long long g = tid; g < groups; g += (long long)gridDim.x * CC_THREADS) {
    if constexpr (VEC == 4) {
      const uchar4 p = *reinterpret_cast<const uchar4*>(pred + g * 4);
      const uchar4 t = *reinterpret_cast<const uchar4*>(truth + g * 4);
      *reinterpret_cast<ushort4*>(bits + g * 4) = make_ushort4(one(p.x, t.x), one(p.y, t.y), one(p.z, t.z), one(p.w, t.w));
    } else {
      bits[g] = one(pred[g], truth[g]);
    }
  }
  if (VEC == 4 && tid < S - groups * 4) {              // the tail
    const long long v = groups * 4 + tid;
    bits[v] = one(pred[v], truth[v]);
  }
}

// one launch: the decision bits of the S voxels of one case (arguments already checked, the table with label_lut_ok)
static int label_decision_bits(const uint8_t* pred, const uint8_t* truth, const uint16_t* lut, size_t S, uint16_t* bits,
                               hipStream_t st) {
  LabelBitsLut l;
  for (int v = 0; v < 256; ++v) l.v[v] = lut[v];
  const bool v4 = (((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(truth)) & 3) |
                   (reinterpret_cast<uintptr_t>(bits) & 7)) == 0;
  const dim3 g(cc_grid(v4 ? (S + 3) / 4 : S, CC_STREAM_BLOCKS)), b(CC_THREADS);
  if (v4) hipLaunchKernelGGL(k_label_bits<4>, g, b, 0, st, pred, truth, bits, (long long)S, l);
  else hipLaunchKernelGGL(k_label_bits<1>, g, b, 0, st, pred, truth, bits, (long long)S, l);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // namespace effq
