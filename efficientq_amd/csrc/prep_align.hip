// effq_prep_align: one volume resampled onto another grid through a general affine (prep.py, --prep_align; the rule is
// stated there and restated in include/effq_hip.h).  m (3 x 4, fp64) maps an output voxel index (d, h, w, 1) to source
// voxel coordinates; per axis a, in fp64 and in this order, nothing fused:
//     s_a = ((m[a][0] d + m[a][1] h) + m[a][2] w) + m[a][3].
// The voxel is inside the field of view when -0.5 <= s_a < n_a - 0.5 on all three axes (n the source extent); outside it
// the output is +0.0f (0 for a label) and no source voxel is read.  Inside it:
//   linear   c = clamp(s_a, 0, n_a - 1), i0 = floor(c), i1 = i0 + (i0 < n_a - 1), l1 = float(c - floor(c)), l0 = 1.0f - l1,
//            the eight neighbours combined in fp32 in the order of k_prep_resample_linear (prep.hip);
//   nearest  the index floor(s_a + 0.5), kept at n_a - 1 at most (the sum may round up to n_a when n_a = 1).
// `inside` receives the number of output voxels inside the field of view: every thread counts its own, one shuffle tree
// per wave, one LDS step per workgroup and one integer atomicAdd per workgroup onto the counter the call zeroed on the
// stream.  Integer adds commute: equal inputs give equal bits; no floating-point atomic, no workgroup waits for another.
//
// The shape of the other prep kernels (prep_rows.h): a thread makes four consecutive w of an output row and stores them
// as one PFloat4 / PByte4, the last OW % 4 of a row one by one; at most PREP_MAX_BLOCKS workgroups stride over the items.
// The row's share of the coordinate, m[a][0] d + m[a][1] h, is formed once per item: 3 fp64 multiplies and 6 adds per
// voxel remain, far below what the gather costs.  The kernel is a gather bound by memory: for a matrix near the axes
// the lanes of a wave read neighbouring w of a few source rows; a permuting matrix strides through the source instead.
// Every index is 32-bit: D H W < 2^31 and OD OH OW < 2^31 are argument checks.
#include <math.h>
#include <type_traits>
#include "common.h"
#include "prep_rows.h"

namespace effq {

struct AlignParams {
  const void* x;
  void* y;
  unsigned long long* inside;
  unsigned n[3];             // source extents D, H, W
  unsigned OD, OH, OW;
  double m[12];
};

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
__device__ __forceinline__ unsigned align_near(double s, unsigned n) {
  const unsigned i = (unsigned)floor(s + 0.5);
  return i < n - 1 ? i : n - 1;
}

template <int MODE>
__global__ __launch_bounds__(PREP_THREADS) void k_prep_align(AlignParams p) {
  using T = typename std::conditional<MODE == EFFQ_PREP_LINEAR, float, uint8_t>::type;
  using V = typename std::conditional<MODE == EFFQ_PREP_LINEAR, PFloat4, PByte4>::type;
  __shared__ unsigned s_count[PREP_WAVES];
  const T* x = static_cast<const T*>(p.x);
  T* y = static_cast<T*>(p.y);
  const unsigned gw = (p.OW + 3) / 4, total = p.OD * p.OH * gw;
  const unsigned H = p.n[1], W = p.n[2];
  unsigned mine = 0;
  for (unsigned e = blockIdx.x * PREP_THREADS + threadIdx.x; e < total; e += gridDim.x * PREP_THREADS) {
    const RowItem r = row_item(e, gw, p.OD, p.OH);
    double row[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) row[a] = p.m[4 * a] * (double)r.d + p.m[4 * a + 1] * (double)r.h;
    T out[4];
#pragma unroll
    for (unsigned u = 0; u < 4; ++u) {
      out[u] = (T)0;
      const unsigned ow = r.w0 + u;
      if (ow >= p.OW) continue;
      double s[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) s[a] = (row[a] + p.m[4 * a + 2] * (double)ow) + p.m[4 * a + 3];
      if (!(in_fov(s[0], p.n[0]) && in_fov(s[1], H) && in_fov(s[2], W))) continue;
      ++mine;
      if constexpr (MODE == EFFQ_PREP_LINEAR) {
        unsigned d0, d1, h0, h1, w0, w1;
        float ld0, ld1, lh0, lh1, lw0, lw1;
        align_axis(s[0], p.n[0], d0, d1, ld0, ld1);
        align_axis(s[1], H, h0, h1, lh0, lh1);
        align_axis(s[2], W, w0, w1, lw0, lw1);
        const T* r00 = x + ((size_t)d0 * H + h0) * W;
        const T* r01 = x + ((size_t)d0 * H + h1) * W;
        const T* r10 = x + ((size_t)d1 * H + h0) * W;
        const T* r11 = x + ((size_t)d1 * H + h1) * W;
        // the order of k_prep_resample_linear: l0d (l0h (l0w v000 + l1w v001) + l1h (...)) + l1d (...), fp32, nothing fused
        const float a = ld0 * (lh0 * (lw0 * r00[w0] + lw1 * r00[w1]) + lh1 * (lw0 * r01[w0] + lw1 * r01[w1]));
        const float b = ld1 * (lh0 * (lw0 * r10[w0] + lw1 * r10[w1]) + lh1 * (lw0 * r11[w0] + lw1 * r11[w1]));
        out[u] = (T)(a + b);
      } else {
        out[u] = x[((size_t)align_near(s[0], p.n[0]) * H + align_near(s[1], H)) * W + align_near(s[2], W)];
      }
    }
    T* dst = y + ((size_t)r.d * p.OH + r.h) * p.OW + r.w0;
    if (r.w0 + 4 <= p.OW) {
      V o;
      o.x = out[0]; o.y = out[1]; o.z = out[2]; o.w = out[3];
      *reinterpret_cast<V*>(dst) = o;
    } else {
      for (unsigned u = 0; r.w0 + u < p.OW; ++u) dst[u] = out[u];
    }
  }
  // every thread of the workgroup arrives here: whole waves enter the butterfly
  mine = wave_sum_all((uint32_t)mine);
  if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long n = 0;
#pragma unroll
    for (int w = 0; w < PREP_WAVES; ++w) n += s_count[w];
    if (n) atomicAdd(p.inside, n);
  }
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_prep_align(const void* x, int D, int H, int W, const double* m, int mode, void* y, int OD, int OH, int OW,
                    long long* inside, void* stream) {
  EFFQ_CHECK_ARG(x && y && m && inside && prep_fits(1, D, H, W) && prep_fits(1, OD, OH, OW));
  EFFQ_CHECK_ARG(mode == EFFQ_PREP_LINEAR || mode == EFFQ_PREP_NEAREST);
  for (int i = 0; i < 12; ++i) EFFQ_CHECK_ARG(isfinite(m[i]));
  EFFQ_CHECK_ARG(mode == EFFQ_PREP_NEAREST || (aligned_to(x, 4) && aligned_to(y, 4)));
  EFFQ_CHECK_ARG(aligned_to(inside, 8));
  AlignParams p;
  p.x = x; p.y = y; p.inside = reinterpret_cast<unsigned long long*>(inside);
  p.n[0] = D; p.n[1] = H; p.n[2] = W; p.OD = OD; p.OH = OH; p.OW = OW;
  for (int i = 0; i < 12; ++i) p.m[i] = m[i];
  const hipStream_t st = as_stream(stream);
  EFFQ_HIP(hipMemsetAsync(inside, 0, sizeof(long long), st));
  const dim3 g(prep_grid((size_t)OD * OH * ((OW + 3) / 4)));
  if (mode == EFFQ_PREP_LINEAR)
    hipLaunchKernelGGL(k_prep_align<EFFQ_PREP_LINEAR>, g, dim3(PREP_THREADS), 0, st, p);
  else
    hipLaunchKernelGGL(k_prep_align<EFFQ_PREP_NEAREST>, g, dim3(PREP_THREADS), 0, st, p);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
