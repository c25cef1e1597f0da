// The sliding window of evaluate.stitched_window_logits (validate_seg, the predict mission): three
// streaming kernels over the window rule of seg_window.h.
//
//   gather  the windows of a volume, each mirrored along the axes of a flip mask, as one channels-last batch
//   put     the network's last head (NCDHW) un-mirrored into the channels-last window buffer, stored or added
//   stitch  the buffer stitched back to the volume: the sum of the covering windows over their count, or with a
//           separable per-axis weight over the weight sum; either divided by the number of passes in the buffer
//
// A flip mask is 0..7: bit 0 mirrors d, bit 1 mirrors h, bit 2 mirrors w; a mirrored axis maps window-local z to p-1-z.
// Every destination element has one owner thread, the covering windows are added in raster order and nothing is reduced
// across threads: no atomics, equal inputs give equal bits.  32-bit index arithmetic on the per-element path (the entry
// points bound the element counts below 2^31: 64-bit division is a long software sequence on the GPU); bounded loops;
// no workgroup waits for another.
#include "common.h"
#include "seg_window.h"

namespace effq {

__device__ __forceinline__ int mirror(int z, int p, int on) { return on ? p - 1 - z : z; }

// ---- gather: vol (N, C, D, H, W) -> out (count, N, pd, ph, pw, C), windows first .. first + count - 1, mirrored ----
template <int VEC>
__global__ __launch_bounds__(256) void k_window_gather(const float* __restrict__ vol, float* __restrict__ out, WinAxes a,
                                                       int N, int C, int first, int flip, uint32_t total) {
  const size_t plane = (size_t)a.D * a.H * a.W;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    uint32_t r = e;
    const int x = (int)(r % a.pw); r /= a.pw;
    const int y = (int)(r % a.ph); r /= a.ph;
    const int z = (int)(r % a.pd); r /= a.pd;
    const int n = (int)(r % N);
    const int win = first + (int)(r / N);
    const int k = win % a.nw, j = (win / a.nw) % a.nh, i = win / (a.nw * a.nh);
    const int d = win_start(i, a.D, a.pd, a.sd) + mirror(z, a.pd, flip & 1);
    const int h = win_start(j, a.H, a.ph, a.sh) + mirror(y, a.ph, flip & 2);
    const int w = win_start(k, a.W, a.pw, a.sw) + mirror(x, a.pw, flip & 4);
    // lanes of a wave hold consecutive x: every channel plane is read coalesced (backwards when w is mirrored, within
    // the same lines), every voxel written as C contiguous floats
    const float* src = vol + (size_t)n * C * plane + ((size_t)d * a.H + h) * a.W + w;
    float* dst = out + (size_t)e * C;
    for (int c = 0; c < C; c += VEC) {
      if constexpr (VEC == 4) {
        float4 v;
        v.x = src[(size_t)c * plane];
        v.y = src[(size_t)(c + 1) * plane];
        v.z = src[(size_t)(c + 2) * plane];
        v.w = src[(size_t)(c + 3) * plane];
        *reinterpret_cast<float4*>(dst + c) = v;
      } else {
        dst[c] = src[(size_t)c * plane];
      }
    }
  }
}

// ---- put: src (count, C, pd, ph, pw) -> dst (count, pd, ph, pw, C), un-mirrored, stored or added ---------------
// One thread per destination voxel e = ((m pd + z) ph + y) pw + x; it owns the C floats at dst + e C.
template <int VEC, bool ACC>
__global__ __launch_bounds__(256) void k_window_put(const float* __restrict__ src, float* __restrict__ dst, int C,
                                                    int pd, int ph, int pw, int flip, uint32_t total) {
  const uint32_t wvox = (uint32_t)pd * ph * pw;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    uint32_t r = e;
    const int x = (int)(r % pw); r /= pw;
    const int y = (int)(r % ph); r /= ph;
    const int z = (int)(r % pd);
    const uint32_t m = r / pd;
    const uint32_t at = ((uint32_t)mirror(z, pd, flip & 1) * ph + mirror(y, ph, flip & 2)) * pw + mirror(x, pw, flip & 4);
    // m C wvox + c wvox + at < count C wvox < 2^31
    const float* s = src + (size_t)(m * C * wvox + at);
    float* o = dst + (size_t)e * C;
    for (int c = 0; c < C; c += VEC) {
      if constexpr (VEC == 4) {
        float4 v;
        v.x = s[(size_t)c * wvox];
        v.y = s[(size_t)(c + 1) * wvox];
        v.z = s[(size_t)(c + 2) * wvox];
        v.w = s[(size_t)(c + 3) * wvox];
        if constexpr (ACC) {
          const float4 old = *reinterpret_cast<const float4*>(o + c);
          v.x = old.x + v.x; v.y = old.y + v.y; v.z = old.z + v.z; v.w = old.w + v.w;
        }
        *reinterpret_cast<float4*>(o + c) = v;
      } else {
        const float v = s[(size_t)c * wvox];
        if constexpr (ACC) o[c] = o[c] + v;
        else o[c] = v;
      }
    }
  }
}

// ---- stitch: win (nwin, N, pd, ph, pw, C) -> out (N, C, D, H, W) --------------------------------------------------
// One thread per output voxel adds the covering windows in raster order onto 0.0f and divides once.  Unweighted: the
// addends, the order and the rounding of evaluate.patch_to_image3d over fn times their count.  WEIGHTED: every addend
// scaled by (wd[z] wh[y]) ww[x], over fn times the weight sum; with weights 1.0f every product is the addend itself and
// the weight sum is the exact count, so the two instances give equal bits.
//
// The loops keep the window rule and the hoisted `c < C` masks in scalar registers, and the scalar registers, not the
// vector ones, set the occupancy here: they are handed out in blocks of 16, so the 98 the unweighted instance would take
// (104 the weighted one) cost the eighth wave per SIMD that 96 still has - measured on the (512, 512, 200) volume as
// 0.94 ms against 0.85 ms, and 1.19 ms against 1.08 ms.  Hence the cap: the compiler moves 2 (8) of them into lanes of
// a vector register, no scratch, and both instances run 8 waves.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(96)))
void k_window_stitch(const float* __restrict__ win, const float* __restrict__ wd, const float* __restrict__ wh,
                     const float* __restrict__ ww, float* __restrict__ out, WinAxes a, int N, int C, float fn,
                     uint32_t total) {
  const size_t plane = (size_t)a.D * a.H * a.W;
  const size_t wvox = (size_t)a.pd * a.ph * a.pw;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    uint32_t r = e;
    const int w = (int)(r % a.W); r /= a.W;
    const int h = (int)(r % a.H); r /= a.H;
    const int d = (int)(r % a.D);
    const int n = (int)(r / a.D);
    float acc[STITCH_MAX_C];
#pragma unroll
    for (int c = 0; c < STITCH_MAX_C; ++c) acc[c] = 0.0f;
    float wsum = 0.0f;
    int cnt = 0;
    for (int i = 0; i < a.nd; ++i) {
      const int z = d - win_start(i, a.D, a.pd, a.sd);
      if (z < 0 || z >= a.pd) continue;
      float gz = 1.0f;
      if constexpr (WEIGHTED) gz = wd[z];
      for (int j = 0; j < a.nh; ++j) {
        const int y = h - win_start(j, a.H, a.ph, a.sh);
        if (y < 0 || y >= a.ph) continue;
        float gzy = gz;
        if constexpr (WEIGHTED) gzy = gz * wh[y];
        for (int k = 0; k < a.nw; ++k) {
          const int x = w - win_start(k, a.W, a.pw, a.sw);
          if (x < 0 || x >= a.pw) continue;
          const size_t widx = ((size_t)(i * a.nh + j) * a.nw + k) * N + n;
          const float* src = win + ((widx * wvox) + ((size_t)z * a.ph + y) * a.pw + x) * C;
          if constexpr (WEIGHTED) {
            const float wgt = gzy * ww[x];
#pragma unroll
            for (int c = 0; c < STITCH_MAX_C; ++c)
              if (c < C) acc[c] = acc[c] + wgt * src[c];
            wsum = wsum + wgt;
          } else {
#pragma unroll
            for (int c = 0; c < STITCH_MAX_C; ++c)
              if (c < C) acc[c] = acc[c] + src[c];
            ++cnt;
          }
        }
      }
    }
    const float den = fn * (WEIGHTED ? wsum : (float)cnt);
    float* dst = out + (size_t)n * C * plane + ((size_t)d * a.H + h) * a.W + w;
#pragma unroll
    for (int c = 0; c < STITCH_MAX_C; ++c)
      if (c < C) dst[(size_t)c * plane] = acc[c] / den;
  }
}

template <int VEC>
static void launch_put(bool acc, unsigned grid, hipStream_t st, const float* src, float* dst, int C, int pd, int ph,
                       int pw, int flip, uint32_t total) {
  if (acc)
    hipLaunchKernelGGL((k_window_put<VEC, true>), dim3(grid), dim3(256), 0, st, src, dst, C, pd, ph, pw, flip, total);
  else
    hipLaunchKernelGGL((k_window_put<VEC, false>), dim3(grid), dim3(256), 0, st, src, dst, C, pd, ph, pw, flip, total);
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_window_gather(const float* vol, int N, int C, int D, int H, int W, int pd, int ph, int pw, int od, int oh,
                       int ow, int first, int count, int flip, float* out, void* stream) {
  EFFQ_CHECK_ARG(vol && out && N > 0 && C > 0 && D > 0 && H > 0 && W > 0);
  EFFQ_CHECK_ARG(flip >= 0 && flip <= 7);
  WinAxes a;
  EFFQ_CHECK_ARG(make_axes(D, H, W, pd, ph, pw, od, oh, ow, a));
  EFFQ_CHECK_ARG(first >= 0 && count > 0 && (long long)first + count <= (long long)a.nd * a.nh * a.nw);
  const size_t total = (size_t)count * N * pd * ph * pw;
  EFFQ_CHECK_ARG(total < (1u << 31));
  const bool v4 = C % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (v4)
    hipLaunchKernelGGL(k_window_gather<4>, dim3(grid_for(total, 1 << 16)), dim3(256), 0, as_stream(stream), vol, out, a,
                       N, C, first, flip, (uint32_t)total);
  else
    hipLaunchKernelGGL(k_window_gather<1>, dim3(grid_for(total, 1 << 16)), dim3(256), 0, as_stream(stream), vol, out, a,
                       N, C, first, flip, (uint32_t)total);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_window_put(const float* src, int count, int C, int pd, int ph, int pw, int flip, int accumulate, float* dst,
                    void* stream) {
  EFFQ_CHECK_ARG(src && dst && count > 0 && C > 0 && C <= STITCH_MAX_C && pd > 0 && ph > 0 && pw > 0);
  EFFQ_CHECK_ARG(flip >= 0 && flip <= 7 && (accumulate == 0 || accumulate == 1));
  // the element count, not only the voxel count, stays below 2^31: the kernel forms source offsets in 32 bits
  const unsigned long long wvox = (unsigned long long)pd * ph * pw;
  EFFQ_CHECK_ARG(wvox < (1ull << 31) && (unsigned long long)count * C * wvox < (1ull << 31));
  const size_t total = (size_t)count * wvox;
  const bool v4 = C % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  const unsigned grid = grid_for(total, 1 << 16);
  if (v4)
    launch_put<4>(accumulate != 0, grid, as_stream(stream), src, dst, C, pd, ph, pw, flip, (uint32_t)total);
  else
    launch_put<1>(accumulate != 0, grid, as_stream(stream), src, dst, C, pd, ph, pw, flip, (uint32_t)total);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_window_stitch(const float* win, int N, int C, int D, int H, int W, int pd, int ph, int pw, int od, int oh,
                       int ow, const float* wd, const float* wh, const float* ww, int nflip, float* out, void* stream) {
  EFFQ_CHECK_ARG(win && out && N > 0 && C > 0 && C <= STITCH_MAX_C && D > 0 && H > 0 && W > 0);
  const bool weighted = wd && wh && ww;
  EFFQ_CHECK_ARG((weighted || (!wd && !wh && !ww)) && nflip >= 1);
  WinAxes a;
  EFFQ_CHECK_ARG(make_axes(D, H, W, pd, ph, pw, od, oh, ow, a));
  const size_t total = (size_t)N * D * H * W;
  EFFQ_CHECK_ARG(total < (1u << 31));
  if (weighted)
    hipLaunchKernelGGL(k_window_stitch<true>, dim3(grid_for(total, 1 << 16)), dim3(256), 0, as_stream(stream), win, wd,
                       wh, ww, out, a, N, C, (float)nflip, (uint32_t)total);
  else
    hipLaunchKernelGGL(k_window_stitch<false>, dim3(grid_for(total, 1 << 16)), dim3(256), 0, as_stream(stream), win, wd,
                       wh, ww, out, a, N, C, (float)nflip, (uint32_t)total);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
