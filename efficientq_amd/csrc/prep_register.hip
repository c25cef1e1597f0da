// The two kernels of --prep_register rigid (register.py; the rule is restated in include/effq_hip.h):
//   effq_prep_bins        a float volume to one uint8 per voxel, its intensity bin 0 .. REG_BINS - 1 or REG_SKIP;
//   effq_prep_joint_hist  the joint histograms of the reference's bins and the bins of the moving volume sampled through K
//                         candidate matrices: the objective of the search, evaluated for all candidates of a step at once.
//
// The sample is the gather of k_prep_align<EFFQ_PREP_LINEAR> to the bit (prep_geom.h: the fp64 coordinates in the same
// order, the same field of view, clamp, weights and order of the eight products), so the transform the search settles on
// is judged on exactly the values the alignment that follows will write.
//
// How the work is split.  A thread owns four consecutive sampled voxels of one row of the reference (prep_rows.h), reads
// their four bins once, and walks the K candidates: per candidate the row's share of the coordinates is formed once, then
// up to four gathers of eight floats.  K gathers per read of the reference and no store: this is why the host batches the
// 13 candidates of a pattern-search step into one launch.  Each workgroup keeps the K histograms in dynamic LDS as uint32,
// K x 1024 x 4 B (52 KB at K = 13, 64 KB at K = 16; a workgroup sees fewer than 2^31 samples, so they cannot wrap), cleared
// at the start, counted by LDS integer atomicAdd; at the end it walks its bins and adds every non-zero one to `hist` with
// one 64-bit integer atomicAdd.  Integer adds commute: equal inputs give equal bits; no floating-point atomic, no workgroup
// waits for another, the host reads nothing inside the call.  `hist` is cleared by a small kernel on the same stream.
//
// Smooth images put the lanes of a wave into few bins, and LDS atomics on one address serialise.  Combining equal
// (bf, bm) of a wave by ballot before the add was measured and is no faster, even on a constant volume (DESIGN section
// 29), so the add is the plain one.
#include <math.h>
#include "common.h"
#include "prep_geom.h"
#include "prep_rows.h"

namespace effq {

constexpr int REG_BINS = EFFQ_PREP_REGISTER_BINS;
constexpr unsigned REG_SKIP = 255;                     // "not sampled"
constexpr int REG_HIST = REG_BINS * REG_BINS;          // the counters of one candidate
constexpr int REG_MAX_K = EFFQ_PREP_REGISTER_MAX_K;
static_assert(REG_BINS < (int)REG_SKIP && REG_MAX_K * REG_HIST * 4 <= 64 * 1024, "the LDS budget of the joint histogram");

// The bin rule, all fp32, nothing fused: t = (v - lo) * scale; a NaN t is not sampled; t < 0 is bin 0, t >= B is bin
// B - 1 (so -Inf and +Inf are the two outer bins), otherwise the bin is (int)t.
__device__ __forceinline__ unsigned reg_bin(float v, float lo, float scale) {
  const float t = (v - lo) * scale;
  if (t != t) return REG_SKIP;
  if (t < 0.0f) return 0u;
  if (t >= (float)REG_BINS) return (unsigned)(REG_BINS - 1);
  return (unsigned)(int)t;
}

struct BinsParams {
  const float* x;
  uint8_t* y;
  unsigned D, H, W;
  float lo, scale;
  int mask_nonzero;
};

__global__ __launch_bounds__(PREP_THREADS) void k_reg_bins(BinsParams p) {
  const unsigned gw = (p.W + 3) / 4, total = p.D * p.H * gw;
  for (unsigned e = blockIdx.x * PREP_THREADS + threadIdx.x; e < total; e += gridDim.x * PREP_THREADS) {
    const RowItem r = row_item(e, gw, p.D, p.H);
    const size_t at = ((size_t)r.d * p.H + r.h) * p.W + r.w0;
    const bool whole = r.w0 + 4 <= p.W;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (whole) {
      const PFloat4 q = *reinterpret_cast<const PFloat4*>(p.x + at);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      for (unsigned u = 0; r.w0 + u < p.W; ++u) v[u] = p.x[at + u];
    }
    uint8_t b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      b[u] = (uint8_t)((p.mask_nonzero && v[u] == 0.0f) ? REG_SKIP : reg_bin(v[u], p.lo, p.scale));
    if (whole) {
      PByte4 o;
      o.x = b[0]; o.y = b[1]; o.z = b[2]; o.w = b[3];
      *reinterpret_cast<PByte4*>(p.y + at) = o;
    } else {
      for (unsigned u = 0; r.w0 + u < p.W; ++u) p.y[at + u] = b[u];
    }
  }
}

struct HistParams {
  const uint8_t* fbin;
  const float* mov;
  unsigned long long* hist;
  unsigned D, H, W;          // the reference grid
  unsigned n[3];             // the moving volume's extents
  unsigned sd, sh, sw;       // the sample stride
  unsigned OD, OH, OW;       // the sampled extents: ceil(D / sd), ...
  int K;
  float lo, scale;
  double m[REG_MAX_K][12];
};

__global__ __launch_bounds__(PREP_THREADS) void k_reg_clear(unsigned long long* hist, unsigned n) {
  const unsigned i = blockIdx.x * PREP_THREADS + threadIdx.x;
  if (i < n) hist[i] = 0ull;
}

__global__ __launch_bounds__(PREP_THREADS) void k_reg_joint_hist(HistParams p) {
  extern __shared__ unsigned s_hist[];                  // [K][REG_BINS][REG_BINS]
  const unsigned cells = (unsigned)p.K * REG_HIST;
  for (unsigned i = threadIdx.x; i < cells; i += PREP_THREADS) s_hist[i] = 0u;
  __syncthreads();
  const unsigned gw = (p.OW + 3) / 4, total = p.OD * p.OH * gw;
  const unsigned MH = p.n[1], MW = p.n[2];
  for (unsigned e = blockIdx.x * PREP_THREADS + threadIdx.x; e < total; e += gridDim.x * PREP_THREADS) {
    const RowItem r = row_item(e, gw, p.OD, p.OH);
    const unsigned d = r.d * p.sd, h = r.h * p.sh;
    const uint8_t* row = p.fbin + ((size_t)d * p.H + h) * p.W;
    unsigned bf[4] = {REG_SKIP, REG_SKIP, REG_SKIP, REG_SKIP};
    if (p.sw == 1 && r.w0 + 4 <= p.OW) {
      const PByte4 q = *reinterpret_cast<const PByte4*>(row + r.w0);
      bf[0] = q.x; bf[1] = q.y; bf[2] = q.z; bf[3] = q.w;
    } else {
      for (unsigned u = 0; u < 4 && r.w0 + u < p.OW; ++u) bf[u] = row[(size_t)(r.w0 + u) * p.sw];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) bf[u] = bf[u] < (unsigned)REG_BINS ? bf[u] : REG_SKIP;      // no bin: never an LDS index
    if ((bf[0] & bf[1] & bf[2] & bf[3]) == REG_SKIP) continue;         // 255 is all ones in a byte: nothing to sample
    for (int k = 0; k < p.K; ++k) {
      const double* m = p.m[k];
      unsigned* hk = s_hist + k * REG_HIST;
      double row3[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) row3[a] = m[4 * a] * (double)d + m[4 * a + 1] * (double)h;
#pragma unroll
      for (unsigned u = 0; u < 4; ++u) {
        if (bf[u] == REG_SKIP) continue;
        const unsigned w = (r.w0 + u) * p.sw;
        double s[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] = (row3[a] + m[4 * a + 2] * (double)w) + m[4 * a + 3];
        if (!(in_fov(s[0], p.n[0]) && in_fov(s[1], MH) && in_fov(s[2], MW))) continue;
        unsigned d0, d1, h0, h1, x0, x1;
        float ld0, ld1, lh0, lh1, lw0, lw1;
        align_axis(s[0], p.n[0], d0, d1, ld0, ld1);
        align_axis(s[1], MH, h0, h1, lh0, lh1);
        align_axis(s[2], MW, x0, x1, lw0, lw1);
        const float* r00 = p.mov + ((size_t)d0 * MH + h0) * MW;
        const float* r01 = p.mov + ((size_t)d0 * MH + h1) * MW;
        const float* r10 = p.mov + ((size_t)d1 * MH + h0) * MW;
        const float* r11 = p.mov + ((size_t)d1 * MH + h1) * MW;
        // the order of k_prep_align: l0d (l0h (l0w v000 + l1w v001) + l1h (...)) + l1d (...), fp32, nothing fused
        const float a = ld0 * (lh0 * (lw0 * r00[x0] + lw1 * r00[x1]) + lh1 * (lw0 * r01[x0] + lw1 * r01[x1]));
        const float b = ld1 * (lh0 * (lw0 * r10[x0] + lw1 * r10[x1]) + lh1 * (lw0 * r11[x0] + lw1 * r11[x1]));
        const unsigned bm = reg_bin(a + b, p.lo, p.scale);
        if (bm != REG_SKIP) atomicAdd(hk + bf[u] * REG_BINS + bm, 1u);
      }
    }
  }
  __syncthreads();
  for (unsigned i = threadIdx.x; i < cells; i += PREP_THREADS) {
    const unsigned c = s_hist[i];
    if (c) atomicAdd(p.hist + i, (unsigned long long)c);
  }
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_prep_bins(const float* x, int D, int H, int W, float lo, float scale, int mask_nonzero, unsigned char* y,
                   void* stream) {
  EFFQ_CHECK_ARG(x && y && prep_fits(1, D, H, W) && aligned_to(x, 4));
  EFFQ_CHECK_ARG(isfinite(lo) && isfinite(scale) && scale > 0.0f && (mask_nonzero == 0 || mask_nonzero == 1));
  BinsParams p;
  p.x = x; p.y = y; p.D = D; p.H = H; p.W = W; p.lo = lo; p.scale = scale; p.mask_nonzero = mask_nonzero;
  hipLaunchKernelGGL(k_reg_bins, dim3(prep_grid((size_t)D * H * ((W + 3) / 4))), dim3(PREP_THREADS), 0, as_stream(stream),
                     p);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_prep_joint_hist(const unsigned char* fbin, int D, int H, int W, const float* mov, int MD, int MH, int MW,
                         const double* m, int K, float lo, float scale, int sd, int sh, int sw, unsigned long long* hist,
                         void* stream) {
  EFFQ_CHECK_ARG(fbin && mov && m && hist && prep_fits(1, D, H, W) && prep_fits(1, MD, MH, MW));
  EFFQ_CHECK_ARG(K >= 1 && K <= REG_MAX_K && sd >= 1 && sh >= 1 && sw >= 1);
  EFFQ_CHECK_ARG(aligned_to(mov, 4) && aligned_to(hist, 8));
  EFFQ_CHECK_ARG(isfinite(lo) && isfinite(scale) && scale > 0.0f);
  for (int i = 0; i < 12 * K; ++i) EFFQ_CHECK_ARG(isfinite(m[i]));
  HistParams p;
  p.fbin = fbin; p.mov = mov; p.hist = hist;
  p.D = D; p.H = H; p.W = W; p.n[0] = MD; p.n[1] = MH; p.n[2] = MW;
  p.sd = sd; p.sh = sh; p.sw = sw;
  p.OD = (D + sd - 1) / sd; p.OH = (H + sh - 1) / sh; p.OW = (W + sw - 1) / sw;
  p.K = K; p.lo = lo; p.scale = scale;
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < 12; ++i) p.m[k][i] = m[12 * k + i];
  const hipStream_t st = as_stream(stream);
  const unsigned cells = (unsigned)K * REG_HIST;
  const size_t lds = (size_t)cells * sizeof(unsigned);
  EFFQ_HIP(raise_lds_limit<k_reg_joint_hist>(lds));
  hipLaunchKernelGGL(k_reg_clear, dim3((cells + PREP_THREADS - 1) / PREP_THREADS), dim3(PREP_THREADS), 0, st, hist, cells);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_reg_joint_hist, dim3(prep_grid((size_t)p.OD * p.OH * ((p.OW + 3) / 4))),
                     dim3(PREP_THREADS), lds, st, p);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
