// The decision bits of one case: decide<MODE, C> of every voxel -> 16 bits per voxel, pred | gt << 8.  One launch for
// the lesion counts (seg_cc.hip) and the surface distances (seg_surface.hip): plane q < C of a case is bit q (the
// predicted mask of class q), plane C + q is bit 8 + q (its label mask).
#pragma once
#include "common.h"
#include "seg_decide.h"

namespace effq {

constexpr int CC_THREADS = 256;
constexpr int CC_STREAM_BLOCKS = 4096;                 // streaming kernels: blocks per plane at most, grid-stride beyond

static inline unsigned cc_grid(size_t items, size_t cap) {
  size_t nb = (items + CC_THREADS - 1) / CC_THREADS;
  if (nb < 1) nb = 1;
  return (unsigned)(nb < cap ? nb : cap);
}

// the bit of plane `plane` of a case with C classes in its decision bits
__device__ __forceinline__ int cc_plane_bit(int plane, int C) { return plane < C ? plane : 8 + plane - C; }

struct CcMaskParams {
  const float* logits;    // (C, S)
  const uint8_t* label;   // (S) class ids for argmax, (C, S) 0/1 for multi-label
  uint16_t* bits;         // (S)
  long long S;
  int fuse;
  float thresh;
};

template <int MODE, int VEC, int C>
__global__ __launch_bounds__(CC_THREADS) void k_cc_masks(CcMaskParams p) {
  const long long groups = p.S / VEC;
  const long long lab_stride = MODE == EFFQ_SEG_ARGMAX ? 0 : p.S;
  for (long long g = (long long)blockIdx.x * CC_THREADS + threadIdx.x; g < groups;
       g += (long long)gridDim.x * CC_THREADS) {
    float v[VEC][C];
    uint8_t lab[VEC][C];
    constexpr int nlab = MODE == EFFQ_SEG_ARGMAX ? 1 : C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if constexpr (VEC == 4) {
        const float4 f = *reinterpret_cast<const float4*>(p.logits + c * p.S + g * 4);
        v[0][c] = f.x; v[1][c] = f.y; v[2][c] = f.z; v[3][c] = f.w;
      } else {
        v[0][c] = p.logits[c * p.S + g];
      }
      if (c < nlab) {
        if constexpr (VEC == 4) {
          const uchar4 l = *reinterpret_cast<const uchar4*>(p.label + c * lab_stride + g * 4);
          lab[0][c] = l.x; lab[1][c] = l.y; lab[2][c] = l.z; lab[3][c] = l.w;
        } else {
          lab[0][c] = p.label[c * lab_stride + g];
        }
      }
    }
    uint16_t b[VEC];
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      uint32_t pred, gt;
      decide<MODE, C>(v[u], lab[u], p.fuse, p.thresh, pred, gt);
      b[u] = (uint16_t)(pred | (gt << 8));
    }
    if constexpr (VEC == 4)
      *reinterpret_cast<ushort4*>(p.bits + g * 4) = make_ushort4(b[0], b[1], b[2], b[3]);
    else
      p.bits[g] = b[0];
  }
}

template <int C>
static void launch_masks(int mode, bool v4, dim3 g, hipStream_t st, const CcMaskParams& p) {
  const dim3 b(CC_THREADS);
  if (mode == EFFQ_SEG_ARGMAX) {
    if (v4) hipLaunchKernelGGL((k_cc_masks<EFFQ_SEG_ARGMAX, 4, C>), g, b, 0, st, p);
    else hipLaunchKernelGGL((k_cc_masks<EFFQ_SEG_ARGMAX, 1, C>), g, b, 0, st, p);
  } else {
    if (v4) hipLaunchKernelGGL((k_cc_masks<EFFQ_SEG_SIGMOID, 4, C>), g, b, 0, st, p);
    else hipLaunchKernelGGL((k_cc_masks<EFFQ_SEG_SIGMOID, 1, C>), g, b, 0, st, p);
  }
}

// one launch: the decision bits of the S voxels of one case (arguments as effq_seg_tallies, already checked)
static int cc_decision_bits(const float* logits, const uint8_t* label, int C, size_t S, int mode, int fuse, float thresh,
                            uint16_t* bits, hipStream_t st) {
  CcMaskParams p;
  p.logits = logits; p.label = label; p.bits = bits; p.S = (long long)S; p.fuse = fuse; p.thresh = thresh;
  const bool v4 = S % 4 == 0 && ((reinterpret_cast<uintptr_t>(logits) & 15) | (reinterpret_cast<uintptr_t>(label) & 3) |
                                 (reinterpret_cast<uintptr_t>(bits) & 7)) == 0;
  const dim3 g(cc_grid(v4 ? S / 4 : S, CC_STREAM_BLOCKS));
  switch (C) {
    case 1: launch_masks<1>(mode, v4, g, st, p); break;
    case 2: launch_masks<2>(mode, v4, g, st, p); break;
    case 3: launch_masks<3>(mode, v4, g, st, p); break;
    case 4: launch_masks<4>(mode, v4, g, st, p); break;
    case 5: launch_masks<5>(mode, v4, g, st, p); break;
    case 6: launch_masks<6>(mode, v4, g, st, p); break;
    case 7: launch_masks<7>(mode, v4, g, st, p); break;
    default: launch_masks<8>(mode, v4, g, st, p); break;
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // namespace effq
