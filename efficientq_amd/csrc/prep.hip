// The device side of the `prep` mission (prep.py): one subject of C modality volumes (C, D, H, W) fp32, S = D H W voxels
// each, is turned into the standardised, cropped arrays the `ptq` mission reads.  Three passes over the subject:
//   1 effq_prep_bbox_moments   the box of the union mask, and per modality the count and the fp64 sum over its own mask;
//   2 effq_prep_sqdev          per modality sum (x - mean)^2 over its mask in fp64, with the mean of pass 1;
//   3 effq_prep_standardise_crop   y = mask ? float((double(x) - mean) / std) : +0.0f inside the crop box.
// The variance takes two passes because CT values lie thousands of units from zero with a spread of tens: sum x^2 -
// n mean^2 in one pass cancels the digits the spread lives in.  Before them, optionally, effq_prep_window (clip in place)
// and effq_prep_resample (one voxel spacing; the anti-alias filter that may go in front of it is prep_smooth.hip); beside
// them effq_prep_crop_u8 (the label) and effq_prep_union_mask.
//
// Streaming, HBM-bound: each thread takes groups of four consecutive voxels with one 16-B load per modality, through a
// type of 4-B alignment since neither the planes (S % 4 != 0) nor the rows of a crop start on 16 B.  Reductions: every
// thread adds its voxels in index order, one shuffle tree per wave, one LDS step per workgroup, per-workgroup partials
// in `ws`, and one finishing workgroup that adds them in block order.  The grid depends on the extents alone and there
// is no floating-point atomic: equal inputs give equal bits.  Every index is 32-bit: C S < 2^31 is an argument check.
#include "common.h"
#include "prep_rows.h"

namespace effq {

constexpr int PREP_MAXC = EFFQ_PREP_MAX_MODALITIES;
// per workgroup: PREP_MAXC sums, PREP_MAXC counts, the six box values
static_assert((size_t)PREP_MAX_BLOCKS * (PREP_MAXC * 8 + PREP_MAXC * 8 + 8 * 4) <= EFFQ_PREP_WS_BYTES, "workspace");

struct PrepWs {
  double* sum;        // (PREP_MAX_BLOCKS, PREP_MAXC)
  long long* cnt;     // (PREP_MAX_BLOCKS, PREP_MAXC)
  int* box;           // (PREP_MAX_BLOCKS, 8): min d, h, w, max d, h, w
};
static inline PrepWs prep_ws(void* ws) {
  PrepWs r;
  r.sum = static_cast<double*>(ws);
  r.cnt = reinterpret_cast<long long*>(r.sum + (size_t)PREP_MAX_BLOCKS * PREP_MAXC);
  r.box = reinterpret_cast<int*>(r.cnt + (size_t)PREP_MAX_BLOCKS * PREP_MAXC);
  return r;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- pass 1 ------------------------------------------------------------------------------------------------------------
struct BoxAcc {
  int lo[3], hi[3];
};

// voxel `i` of the grid is inside the union mask
__device__ __forceinline__ void box_add(BoxAcc& b, unsigned i, unsigned H, unsigned W) {
  const unsigned row = i / W, w = i - row * W, d = row / H, h = row - d * H;
  b.lo[0] = min(b.lo[0], (int)d); b.hi[0] = max(b.hi[0], (int)d);
  b.lo[1] = min(b.lo[1], (int)h); b.hi[1] = max(b.hi[1], (int)h);
  b.lo[2] = min(b.lo[2], (int)w); b.hi[2] = max(b.hi[2], (int)w);
}

template <int C>
__global__ __launch_bounds__(PREP_THREADS) void k_prep_bbox_moments(const float* __restrict__ x, unsigned S, unsigned H,
                                                                    unsigned W, int mask_mode, PrepWs ws) {
  double sum[C];
  unsigned cnt[C];            // a thread sees at most S / 4 / gridDim.x * 4 + 1 voxels
  BoxAcc b;
#pragma unroll
  for (int c = 0; c < C; ++c) { sum[c] = 0.0; cnt[c] = 0; }
#pragma unroll
  for (int a = 0; a < 3; ++a) { b.lo[a] = 0x7fffffff; b.hi[a] = -1; }
  const unsigned groups = S / 4;
  for (unsigned g = blockIdx.x * PREP_THREADS + threadIdx.x; g < groups; g += gridDim.x * PREP_THREADS) {
    bool any[4] = {false, false, false, false};
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const PFloat4 v4 = *reinterpret_cast<const PFloat4*>(x + (size_t)c * S + (size_t)g * 4);
      const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool m = in_mask(v[u], mask_mode);
        sum[c] += m ? (double)v[u] : 0.0;
        cnt[c] += m ? 1u : 0u;
        any[u] |= m;
      }
    }
    if (mask_mode == 0) {     // with every voxel inside, the box is the grid: k_prep_moments_final writes it
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (any[u]) box_add(b, g * 4 + u, H, W);
    }
  }
  // the last S % 4 voxels, one each for the first threads of workgroup 0, after their own groups
  const unsigned t = groups * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < S) {
    bool any = false;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float v = x[(size_t)c * S + t];
      const bool m = in_mask(v, mask_mode);
      sum[c] += m ? (double)v : 0.0;
      cnt[c] += m ? 1u : 0u;
      any |= m;
    }
    if (mask_mode == 0 && any) box_add(b, t, H, W);
  }
  __shared__ double rs[PREP_WAVES][C];
  __shared__ unsigned rc[PREP_WAVES][C];
  __shared__ int rb[PREP_WAVES][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double s = wave_sum_all(sum[c]);
    const unsigned n = wave_sum_all(cnt[c]);
    if (lane == 0) { rs[wave][c] = s; rc[wave][c] = n; }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int lo = wave_min(b.lo[a]), hi = wave_max(b.hi[a]);
    if (lane == 0) { rb[wave][a] = lo; rb[wave][3 + a] = hi; }
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < C) {
    double s = rs[0][k];
    long long n = rc[0][k];
    for (int w = 1; w < PREP_WAVES; ++w) { s += rs[w][k]; n += rc[w][k]; }
    ws.sum[(size_t)blockIdx.x * PREP_MAXC + k] = s;
    ws.cnt[(size_t)blockIdx.x * PREP_MAXC + k] = n;
  }
  if (k >= 64 && k < 70) {
    const int a = k - 64;
    int v = rb[0][a];
    for (int w = 1; w < PREP_WAVES; ++w) v = a < 3 ? min(v, rb[w][a]) : max(v, rb[w][a]);
    ws.box[(size_t)blockIdx.x * 8 + a] = v;
  }
}

// One workgroup: thread t adds the partials of blocks t, t + 256, ... in that order, then the fixed wave and LDS trees.
// sum_out may be the squared deviations of pass 2 (bbox_out and count_out null).
__global__ __launch_bounds__(PREP_THREADS) void k_prep_moments_final(PrepWs ws, int nblocks, int C, int mask_mode, int D,
                                                                     int H, int W, int* __restrict__ bbox_out,
                                                                     long long* __restrict__ count_out,
                                                                     double* __restrict__ sum_out) {
  __shared__ double rs[PREP_WAVES][PREP_MAXC];
  __shared__ long long rc[PREP_WAVES][PREP_MAXC];
  __shared__ int rb[PREP_WAVES][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = 0; c < C; ++c) {
    double s = 0.0;
    long long n = 0;
    for (int blk = threadIdx.x; blk < nblocks; blk += PREP_THREADS) {
      s += ws.sum[(size_t)blk * PREP_MAXC + c];
      if (count_out) n += ws.cnt[(size_t)blk * PREP_MAXC + c];
    }
    s = wave_sum_all(s);
    const long long nn = wave_sum_all(n);
    if (lane == 0) { rs[wave][c] = s; rc[wave][c] = nn; }
  }
  if (bbox_out) {
    for (int a = 0; a < 6; ++a) {
      int v = a < 3 ? 0x7fffffff : -1;
      for (int blk = threadIdx.x; blk < nblocks; blk += PREP_THREADS) {
        const int q = ws.box[(size_t)blk * 8 + a];
        v = a < 3 ? min(v, q) : max(v, q);
      }
      v = a < 3 ? wave_min(v) : wave_max(v);
      if (lane == 0) rb[wave][a] = v;
    }
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < C) {
    double s = rs[0][k];
    long long n = rc[0][k];
    for (int w = 1; w < PREP_WAVES; ++w) { s += rs[w][k]; n += rc[w][k]; }
    sum_out[k] = s;
    if (count_out) count_out[k] = n;
  }
  if (bbox_out && k >= 64 && k < 70) {
    const int a = k - 64;
    int v = rb[0][a];
    for (int w = 1; w < PREP_WAVES; ++w) v = a < 3 ? min(v, rb[w][a]) : max(v, rb[w][a]);
    const int ext[3] = {D, H, W};
    if (mask_mode != 0) v = a < 3 ? 0 : ext[a - 3] - 1;
    else if (a < 3 && v == 0x7fffffff) v = ext[a];          // empty union mask: min = extent > max = -1
    bbox_out[a] = v;
  }
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(PREP_THREADS) void k_prep_sqdev(const float* __restrict__ x, unsigned S, int mask_mode,
                                                             const double* __restrict__ mean, PrepWs ws) {
  double mu[C], sum[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { mu[c] = mean[c]; sum[c] = 0.0; }
  const unsigned groups = S / 4;
  for (unsigned g = blockIdx.x * PREP_THREADS + threadIdx.x; g < groups; g += gridDim.x * PREP_THREADS) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const PFloat4 v4 = *reinterpret_cast<const PFloat4*>(x + (size_t)c * S + (size_t)g * 4);
      const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double d = (double)v[u] - mu[c];
        sum[c] += in_mask(v[u], mask_mode) ? d * d : 0.0;
      }
    }
  }
  const unsigned t = groups * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < S) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float v = x[(size_t)c * S + t];
      const double d = (double)v - mu[c];
      sum[c] += in_mask(v, mask_mode) ? d * d : 0.0;
    }
  }
  __shared__ double rs[PREP_WAVES][C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double s = wave_sum_all(sum[c]);
    if (lane == 0) rs[wave][c] = s;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < C) {
    double s = rs[0][k];
    for (int w = 1; w < PREP_WAVES; ++w) s += rs[w][k];
    ws.sum[(size_t)blockIdx.x * PREP_MAXC + k] = s;
  }
}

// ---- pass 3 and the other row-wise kernels ----------------------------------------------------------------------------
// A thread takes four consecutive w of one output row (row_item of prep_rows.h).
struct CropParams {
  const void* x;
  void* y;
  const double* mean;
  const double* std;
  unsigned C, D, H, W, OD, OH, OW;
  unsigned p0, p1, p2;      // the low corner of the box
  int mask_mode;
};

__device__ __forceinline__ float standardise(float v, double mu, double sd, int mask_mode) {
  return in_mask(v, mask_mode) ? (float)(((double)v - mu) / sd) : 0.0f;
}

__global__ __launch_bounds__(PREP_THREADS) void k_prep_standardise_crop(CropParams p) {
  const unsigned gw = (p.OW + 3) / 4, total = p.C * p.OD * p.OH * gw;
  const float* x = static_cast<const float*>(p.x);
  float* y = static_cast<float*>(p.y);
  for (unsigned e = blockIdx.x * PREP_THREADS + threadIdx.x; e < total; e += gridDim.x * PREP_THREADS) {
    const RowItem r = row_item(e, gw, p.OD, p.OH);
    const double mu = p.mean[r.n], sd = p.std[r.n];
    const float* src = x + (((size_t)r.n * p.D + r.d + p.p0) * p.H + r.h + p.p1) * p.W + p.p2 + r.w0;
    float* dst = y + (((size_t)r.n * p.OD + r.d) * p.OH + r.h) * p.OW + r.w0;
    if (r.w0 + 4 <= p.OW) {
      const PFloat4 v = *reinterpret_cast<const PFloat4*>(src);
      PFloat4 o;
      o.x = standardise(v.x, mu, sd, p.mask_mode); o.y = standardise(v.y, mu, sd, p.mask_mode);
      o.z = standardise(v.z, mu, sd, p.mask_mode); o.w = standardise(v.w, mu, sd, p.mask_mode);
      *reinterpret_cast<PFloat4*>(dst) = o;
    } else {
      for (unsigned u = 0; r.w0 + u < p.OW; ++u) dst[u] = standardise(src[u], mu, sd, p.mask_mode);
    }
  }
}

__global__ __launch_bounds__(PREP_THREADS) void k_prep_crop_u8(CropParams p) {
  const unsigned gw = (p.OW + 3) / 4, total = p.C * p.OD * p.OH * gw;
  const uint8_t* x = static_cast<const uint8_t*>(p.x);
  uint8_t* y = static_cast<uint8_t*>(p.y);
  for (unsigned e = blockIdx.x * PREP_THREADS + threadIdx.x; e < total; e += gridDim.x * PREP_THREADS) {
    const RowItem r = row_item(e, gw, p.OD, p.OH);
    const uint8_t* src = x + (((size_t)r.n * p.D + r.d + p.p0) * p.H + r.h + p.p1) * p.W + p.p2 + r.w0;
    uint8_t* dst = y + (((size_t)r.n * p.OD + r.d) * p.OH + r.h) * p.OW + r.w0;
    if (r.w0 + 4 <= p.OW)
      *reinterpret_cast<PByte4*>(dst) = *reinterpret_cast<const PByte4*>(src);
    else
      for (unsigned u = 0; r.w0 + u < p.OW; ++u) dst[u] = src[u];
  }
}

template <int C>
__global__ __launch_bounds__(PREP_THREADS) void k_prep_union_mask(const float* __restrict__ x, unsigned S, int mask_mode,
                                                                  uint8_t* __restrict__ m) {
  const unsigned groups = S / 4;
  for (unsigned g = blockIdx.x * PREP_THREADS + threadIdx.x; g < groups; g += gridDim.x * PREP_THREADS) {
    bool any[4] = {false, false, false, false};
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const PFloat4 v = *reinterpret_cast<const PFloat4*>(x + (size_t)c * S + (size_t)g * 4);
      any[0] |= in_mask(v.x, mask_mode); any[1] |= in_mask(v.y, mask_mode);
      any[2] |= in_mask(v.z, mask_mode); any[3] |= in_mask(v.w, mask_mode);
    }
    PByte4 o;
    o.x = any[0]; o.y = any[1]; o.z = any[2]; o.w = any[3];
    *reinterpret_cast<PByte4*>(m + (size_t)g * 4) = o;
  }
  const unsigned t = groups * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < S) {
    bool any = false;
#pragma unroll
    for (int c = 0; c < C; ++c) any |= in_mask(x[(size_t)c * S + t], mask_mode);
    m[t] = any;
  }
}

__global__ __launch_bounds__(PREP_THREADS) void k_prep_window(float* __restrict__ x, size_t n, float lo, float hi) {
  auto clip = [&](float v) { return v < lo ? lo : (v > hi ? hi : v); };      // numpy.clip: a NaN stays a NaN
  const size_t groups = n / 4;
  for (size_t g = (size_t)blockIdx.x * PREP_THREADS + threadIdx.x; g < groups; g += (size_t)gridDim.x * PREP_THREADS) {
    PFloat4 v = *reinterpret_cast<const PFloat4*>(x + g * 4);
    v.x = clip(v.x); v.y = clip(v.y); v.z = clip(v.z); v.w = clip(v.w);
    *reinterpret_cast<PFloat4*>(x + g * 4) = v;
  }
  const size_t t = groups * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) x[t] = clip(x[t]);
}

// ---- resampling --------------------------------------------------------------------------------------------------------
struct ResampleParams {
  const void* x;
  void* y;
  unsigned N, D, H, W, OD, OH, OW;
  double fd, fh, fw;
};

// output index o of an axis of source extent `in`: s = (o + 0.5) f - 0.5 in fp64, clamped to [0, in - 1]
__device__ __forceinline__ void lin_axis(unsigned o, double f, unsigned in, unsigned& i0, unsigned& i1, float& l0,
                                         float& l1) {
  double s = ((double)o + 0.5) * f - 0.5;
  const double top = (double)(in - 1);
  s = s < 0.0 ? 0.0 : (s > top ? top : s);
  const double fl = floor(s);
  i0 = (unsigned)fl;
  i1 = i0 + (i0 < in - 1 ? 1u : 0u);
  l1 = (float)(s - fl);
  l0 = 1.0f - l1;
}
__device__ __forceinline__ unsigned near_axis(unsigned o, double f, unsigned in) {
  const double s = floor(((double)o + 0.5) * f), top = (double)(in - 1);
  return (unsigned)(s > top ? top : s);
}

__global__ __launch_bounds__(PREP_THREADS) void k_prep_resample_linear(ResampleParams p) {
  const unsigned gw = (p.OW + 3) / 4, total = p.N * p.OD * p.OH * gw;
  const float* x = static_cast<const float*>(p.x);
  float* y = static_cast<float*>(p.y);
  for (unsigned e = blockIdx.x * PREP_THREADS + threadIdx.x; e < total; e += gridDim.x * PREP_THREADS) {
    const RowItem r = row_item(e, gw, p.OD, p.OH);
    unsigned d0, d1, h0, h1;
    float ld0, ld1, lh0, lh1;
    lin_axis(r.d, p.fd, p.D, d0, d1, ld0, ld1);
    lin_axis(r.h, p.fh, p.H, h0, h1, lh0, lh1);
    const float* r00 = x + (((size_t)r.n * p.D + d0) * p.H + h0) * p.W;
    const float* r01 = x + (((size_t)r.n * p.D + d0) * p.H + h1) * p.W;
    const float* r10 = x + (((size_t)r.n * p.D + d1) * p.H + h0) * p.W;
    const float* r11 = x + (((size_t)r.n * p.D + d1) * p.H + h1) * p.W;
    float out[4];
#pragma unroll
    for (unsigned u = 0; u < 4; ++u) {
      const unsigned ow = min(r.w0 + u, p.OW - 1);
      unsigned w0, w1;
      float lw0, lw1;
      lin_axis(ow, p.fw, p.W, w0, w1, lw0, lw1);
      // the order of resample.hip: l0d (l0h (l0w v000 + l1w v001) + l1h (...)) + l1d (...), fp32, nothing fused
      const float a = ld0 * (lh0 * (lw0 * r00[w0] + lw1 * r00[w1]) + lh1 * (lw0 * r01[w0] + lw1 * r01[w1]));
      const float b = ld1 * (lh0 * (lw0 * r10[w0] + lw1 * r10[w1]) + lh1 * (lw0 * r11[w0] + lw1 * r11[w1]));
      out[u] = a + b;
    }
    float* dst = y + (((size_t)r.n * p.OD + r.d) * p.OH + r.h) * p.OW + r.w0;
    if (r.w0 + 4 <= p.OW) {
      PFloat4 o;
      o.x = out[0]; o.y = out[1]; o.z = out[2]; o.w = out[3];
      *reinterpret_cast<PFloat4*>(dst) = o;
    } else {
      for (unsigned u = 0; r.w0 + u < p.OW; ++u) dst[u] = out[u];
    }
  }
}

__global__ __launch_bounds__(PREP_THREADS) void k_prep_resample_nearest(ResampleParams p) {
  const unsigned gw = (p.OW + 3) / 4, total = p.N * p.OD * p.OH * gw;
  const uint8_t* x = static_cast<const uint8_t*>(p.x);
  uint8_t* y = static_cast<uint8_t*>(p.y);
  for (unsigned e = blockIdx.x * PREP_THREADS + threadIdx.x; e < total; e += gridDim.x * PREP_THREADS) {
    const RowItem r = row_item(e, gw, p.OD, p.OH);
    const uint8_t* row = x + (((size_t)r.n * p.D + near_axis(r.d, p.fd, p.D)) * p.H + near_axis(r.h, p.fh, p.H)) * p.W;
    uint8_t out[4];
#pragma unroll
    for (unsigned u = 0; u < 4; ++u) out[u] = row[near_axis(min(r.w0 + u, p.OW - 1), p.fw, p.W)];
    uint8_t* dst = y + (((size_t)r.n * p.OD + r.d) * p.OH + r.h) * p.OW + r.w0;
    if (r.w0 + 4 <= p.OW) {
      PByte4 o;
      o.x = out[0]; o.y = out[1]; o.z = out[2]; o.w = out[3];
      *reinterpret_cast<PByte4*>(dst) = o;
    } else {
      for (unsigned u = 0; r.w0 + u < p.OW; ++u) dst[u] = out[u];
    }
  }
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_prep_window(float* x, size_t n, float lo, float hi, void* stream) {
  EFFQ_CHECK_ARG(x && n > 0 && aligned_to(x, 4) && lo <= hi);       // a NaN bound fails lo <= hi
  hipLaunchKernelGGL(k_prep_window, dim3(prep_grid(n / 4)), dim3(PREP_THREADS), 0, as_stream(stream), x, n, lo, hi);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_prep_resample(const void* x, int N, int D, int H, int W, double fd, double fh, double fw, int mode, void* y,
                       int OD, int OH, int OW, void* stream) {
  EFFQ_CHECK_ARG(x && y && prep_fits(N, D, H, W) && prep_fits(N, OD, OH, OW));
  EFFQ_CHECK_ARG(mode == EFFQ_PREP_LINEAR || mode == EFFQ_PREP_NEAREST);
  EFFQ_CHECK_ARG(fd > 0.0 && fh > 0.0 && fw > 0.0 && fd <= 1e6 && fh <= 1e6 && fw <= 1e6);    // false for a NaN
  EFFQ_CHECK_ARG(mode == EFFQ_PREP_NEAREST || (aligned_to(x, 4) && aligned_to(y, 4)));
  ResampleParams p;
  p.x = x; p.y = y; p.N = N; p.D = D; p.H = H; p.W = W; p.OD = OD; p.OH = OH; p.OW = OW; p.fd = fd; p.fh = fh; p.fw = fw;
  const dim3 g(prep_grid((size_t)N * OD * OH * ((OW + 3) / 4)));
  if (mode == EFFQ_PREP_LINEAR)
    hipLaunchKernelGGL(k_prep_resample_linear, g, dim3(PREP_THREADS), 0, as_stream(stream), p);
  else
    hipLaunchKernelGGL(k_prep_resample_nearest, g, dim3(PREP_THREADS), 0, as_stream(stream), p);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_prep_bbox_moments(const float* x, int C, int D, int H, int W, int mask_mode, int* bbox_out, long long* count_out,
                           double* sum_out, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(x && bbox_out && count_out && sum_out && ws && C <= PREP_MAXC && prep_fits(C, D, H, W));
  EFFQ_CHECK_ARG(mask_mode == EFFQ_PREP_MASK_NONZERO || mask_mode == EFFQ_PREP_MASK_ALL);
  EFFQ_CHECK_ARG(ws_bytes >= EFFQ_PREP_WS_BYTES && aligned_to(x, 4) && aligned_to(ws, 8));
  const unsigned S = (unsigned)D * H * W, nb = prep_grid(S / 4);
  const PrepWs w = prep_ws(ws);
  const hipStream_t st = as_stream(stream);
  const dim3 g(nb), t(PREP_THREADS);
  switch (C) {
    case 1: hipLaunchKernelGGL(k_prep_bbox_moments<1>, g, t, 0, st, x, S, (unsigned)H, (unsigned)W, mask_mode, w); break;
    case 2: hipLaunchKernelGGL(k_prep_bbox_moments<2>, g, t, 0, st, x, S, (unsigned)H, (unsigned)W, mask_mode, w); break;
    case 3: hipLaunchKernelGGL(k_prep_bbox_moments<3>, g, t, 0, st, x, S, (unsigned)H, (unsigned)W, mask_mode, w); break;
    default: hipLaunchKernelGGL(k_prep_bbox_moments<4>, g, t, 0, st, x, S, (unsigned)H, (unsigned)W, mask_mode, w); break;
  }
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_prep_moments_final, dim3(1), t, 0, st, w, (int)nb, C, mask_mode, D, H, W, bbox_out, count_out,
                     sum_out);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_prep_sqdev(const float* x, int C, long long S, int mask_mode, const double* mean, double* sqdev_out, void* ws,
                    size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(x && mean && sqdev_out && ws && C <= PREP_MAXC && prep_fits_flat(C, S));
  EFFQ_CHECK_ARG(mask_mode == EFFQ_PREP_MASK_NONZERO || mask_mode == EFFQ_PREP_MASK_ALL);
  EFFQ_CHECK_ARG(ws_bytes >= EFFQ_PREP_WS_BYTES && aligned_to(x, 4) && aligned_to(ws, 8) && aligned_to(mean, 8));
  const unsigned nb = prep_grid((size_t)S / 4);
  const PrepWs w = prep_ws(ws);
  const hipStream_t st = as_stream(stream);
  const dim3 g(nb), t(PREP_THREADS);
  switch (C) {
    case 1: hipLaunchKernelGGL(k_prep_sqdev<1>, g, t, 0, st, x, (unsigned)S, mask_mode, mean, w); break;
    case 2: hipLaunchKernelGGL(k_prep_sqdev<2>, g, t, 0, st, x, (unsigned)S, mask_mode, mean, w); break;
    case 3: hipLaunchKernelGGL(k_prep_sqdev<3>, g, t, 0, st, x, (unsigned)S, mask_mode, mean, w); break;
    default: hipLaunchKernelGGL(k_prep_sqdev<4>, g, t, 0, st, x, (unsigned)S, mask_mode, mean, w); break;
  }
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_prep_moments_final, dim3(1), t, 0, st, w, (int)nb, C, mask_mode, 0, 0, 0, (int*)nullptr,
                     (long long*)nullptr, sqdev_out);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

static int crop_params(CropParams& p, const void* x, int C, int D, int H, int W, const int* pmin, const int* pmax,
                       void* y) {
  EFFQ_CHECK_ARG(x && y && pmin && pmax && prep_fits(C, D, H, W));
  const int ext[3] = {D, H, W};
  for (int a = 0; a < 3; ++a) EFFQ_CHECK_ARG(0 <= pmin[a] && pmin[a] < pmax[a] && pmax[a] <= ext[a]);
  p.x = x; p.y = y; p.C = C; p.D = D; p.H = H; p.W = W;
  p.p0 = pmin[0]; p.p1 = pmin[1]; p.p2 = pmin[2];
  p.OD = pmax[0] - pmin[0]; p.OH = pmax[1] - pmin[1]; p.OW = pmax[2] - pmin[2];
  p.mean = p.std = nullptr;
  p.mask_mode = EFFQ_PREP_MASK_ALL;
  return EFFQ_OK;
}

int effq_prep_standardise_crop(const float* x, int C, int D, int H, int W, int mask_mode, const int* pmin,
                               const int* pmax, const double* mean, const double* stdev, float* y, void* stream) {
  CropParams p;
  const int rc = crop_params(p, x, C, D, H, W, pmin, pmax, y);
  if (rc != EFFQ_OK) return rc;
  EFFQ_CHECK_ARG(mean && stdev && aligned_to(x, 4) && aligned_to(y, 4) && aligned_to(mean, 8) && aligned_to(stdev, 8));
  EFFQ_CHECK_ARG(mask_mode == EFFQ_PREP_MASK_NONZERO || mask_mode == EFFQ_PREP_MASK_ALL);
  p.mean = mean; p.std = stdev; p.mask_mode = mask_mode;
  const dim3 g(prep_grid((size_t)C * p.OD * p.OH * ((p.OW + 3) / 4)));
  hipLaunchKernelGGL(k_prep_standardise_crop, g, dim3(PREP_THREADS), 0, as_stream(stream), p);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_prep_crop_u8(const uint8_t* x, int C, int D, int H, int W, const int* pmin, const int* pmax, uint8_t* y,
                      void* stream) {
  CropParams p;
  const int rc = crop_params(p, x, C, D, H, W, pmin, pmax, y);
  if (rc != EFFQ_OK) return rc;
  const dim3 g(prep_grid((size_t)C * p.OD * p.OH * ((p.OW + 3) / 4)));
  hipLaunchKernelGGL(k_prep_crop_u8, g, dim3(PREP_THREADS), 0, as_stream(stream), p);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_prep_union_mask(const float* x, int C, long long S, int mask_mode, uint8_t* mask, void* stream) {
  EFFQ_CHECK_ARG(x && mask && C <= PREP_MAXC && prep_fits_flat(C, S) && aligned_to(x, 4));
  EFFQ_CHECK_ARG(mask_mode == EFFQ_PREP_MASK_NONZERO || mask_mode == EFFQ_PREP_MASK_ALL);
  const hipStream_t st = as_stream(stream);
  const dim3 g(prep_grid((size_t)S / 4)), t(PREP_THREADS);
  switch (C) {
    case 1: hipLaunchKernelGGL(k_prep_union_mask<1>, g, t, 0, st, x, (unsigned)S, mask_mode, mask); break;
    case 2: hipLaunchKernelGGL(k_prep_union_mask<2>, g, t, 0, st, x, (unsigned)S, mask_mode, mask); break;
    case 3: hipLaunchKernelGGL(k_prep_union_mask<3>, g, t, 0, st, x, (unsigned)S, mask_mode, mask); break;
    default: hipLaunchKernelGGL(k_prep_union_mask<4>, g, t, 0, st, x, (unsigned)S, mask_mode, mask); break;
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
