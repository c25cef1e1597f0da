// What the two distance transforms share (seg_surface.hip in integers, seg_surface_mm.hip with per-axis weights): the
// surface stencil on the decision bits of seg_masks.h, where the sites of a plane come from, and the size of the LDS slab
// of the line passes.
#pragma once
#include "seg_masks.h"

namespace effq {

// slab of the line passes: tw lines adjacent along w are narrowed down until (n + 2) * tw words fit this.  32 KB keeps
// five workgroups on a compute unit (DESIGN section 13 measured the integer passes with it); a line longer than 2046
// leaves one line per workgroup
constexpr int EDT_LDS_AIM = 32 * 1024;

// the surface bits of one case: a voxel of a mask is a surface voxel when a face neighbour is background or lies outside
// the volume; all 2 C masks at once on the decision bits.  Shared by the integer and the weighted distance transform
// (seg_surface.hip, seg_surface_mm.hip): one definition of S(M).  Internal linkage: each of the two files has its own.
static __global__ __launch_bounds__(CC_THREADS) void k_surf_bits(const uint16_t* __restrict__ bits,
                                                          uint16_t* __restrict__ surf, int D, int H, int W) {
  const int S = D * H * W, HW = H * W;
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)i;
    const uint32_t b = bits[v];
    uint32_t inner = 0;
    if (b) {
      const int w = v % W, q = v / W, h = q % H, d = q / H;
      inner = b;
      inner &= w > 0 ? bits[v - 1] : 0u;
      inner &= w < W - 1 ? bits[v + 1] : 0u;
      inner &= h > 0 ? bits[v - W] : 0u;
      inner &= h < H - 1 ? bits[v + W] : 0u;
      inner &= d > 0 ? bits[v - HW] : 0u;
      inner &= d < D - 1 ? bits[v + HW] : 0u;
    }
    surf[v] = (uint16_t)(b & ~inner);
  }
}

// where the sites of plane q come from: P masks of uint8, or bit cc_plane_bit(q, C) of the surface bits
struct EdtSrc {
  const uint8_t* masks;
  const uint16_t* surf;
  int C;
};

__device__ __forceinline__ bool edt_site(const EdtSrc& s, int plane, int S, int idx) {
  if (s.surf) return (s.surf[idx] >> cc_plane_bit(plane, s.C)) & 1;
  return s.masks[(size_t)plane * S + idx] != 0;
}

}  // namespace effq
