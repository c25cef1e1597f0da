// The kernels of --prep_denoise nlmM (denoise.py, where the rule stands; restated in include/effq_hip.h):
//   effq_prep_denoise_residual   r = |v - mean of the six face neighbours| where all seven lie in Omega, +0 elsewhere;
//   effq_prep_denoise_nlm        the non-local means filter with patch radius 1 and search radius M, and the two sums.
//
// The filter.  A workgroup of NLM_THREADS = 512 owns an output tile of TD x TH x TW = 8 x 8 x 62 voxels, W fastest.  It
// stages the tile plus a halo of M + 1 voxels in LDS once, the edge clamp applied while staging, so that LDS[x] =
// v[clamp(x)] for every extended coordinate x and every patch read below is a plain LDS read:
//   (8 + 2M + 2) x (8 + 2M + 2) x (62 + 2M + 2) floats: 38 KB at M = 1, 72 KB at M = 3, 118 KB at M = 5
// (4, 2 and 1 workgroups of 8 waves per compute unit of 160 KB).  Wave h of the workgroup owns row h of the tile, lane l
// the column w = l - 1: lanes 0 and 63 are the halo columns of the W sum and write nothing.  A thread owns the TD outputs
// of its (h, w) and marches along D.  For one displacement t and one plane d' = -1 .. TD of the tile plus 1:
//   c  = s(d', h - 1, w) + s(d', h, w) + s(d', h + 1, w),   s(x) = (LDS[x] - LDS[x + t])^2       the H sum, in the thread:
//        the three LDS[x] of every plane are read once per tile and stay in registers for all displacements, the three
//        LDS[x + t] are the only LDS reads of the step;
//   P  = (c(w - 1) + c(w)) + c(w + 1)                                                            the W sum, between lanes;
//   S  = (P(d - 1) + P(d)) + P(d + 1)                                                            the D sum, three rolling
//        registers: additions only, nothing is ever subtracted from a running sum.
// That is 3 subtractions, 3 multiply-adds, 2 lane exchanges and 4 additions per voxel and displacement (times 10 / 8
// for the two extra planes) instead of 27 + 27 + 26.  The weight is exp2(min(k0 + k1 S, 0)) with k0 = 2 log2(e) / H2 and
// k1 = -log2(e) / (27 H2 sigma^2) folded on the host in fp64: __builtin_amdgcn_exp2f, the v_exp_f32 instruction, 1 ulp by
// the CDNA3 instruction set guide, results below 2^-126 flushed to 0.  The thread accumulates, in the fixed order of t
// (d slowest, w fastest), den += w and num += w (v_j - v_i): y = v_i + num / (den + wmax) is the rule's quotient with
// v_i taken out, so that every rounding scales with the spread of the window and not with the level of v.
//
// Small weights.  The rule's result depends on the ratios w_j / wmax alone, so fp32 weights are good while wmax is not
// small.  A voxel that has candidates but wmax < 2^-16 (an outlier whose patch resembles nothing) is done again by its
// thread, 27 terms per candidate in fp64 from LDS: a = the exponent, a candidate counts where fp64 exp(-a) > 0, the
// weights are exp(-(a - amin)) and wmax is 1; no candidate left gives y = v_i.
//
// The symmetry w(i, i + t) = w(i + t, i) is not used: the far end of a pair belongs to another thread, mostly of another
// wave, so serving it means a read-modify-write of two accumulators in LDS per pair against one exp2 saved (DESIGN
// section 31).  No floating-point atomic, the grid depends on the extents alone: equal inputs give equal bits.  The two
// sums go through per-workgroup fp64 partials and one finishing workgroup in block order, as in prep.hip.
#include <math.h>
#include "common.h"
#include "prep_rows.h"

namespace effq {

constexpr int NLM_TD = EFFQ_PREP_DENOISE_TILE_D, NLM_TH = EFFQ_PREP_DENOISE_TILE_H, NLM_TW = EFFQ_PREP_DENOISE_TILE_W;
constexpr int NLM_WAVES = NLM_TH, NLM_THREADS = 64 * NLM_WAVES;
constexpr int NLM_MAX_M = 5;
constexpr double NLM_H2 = 1.0;                  // H2 of denoise.py
constexpr float NLM_SMALL = 1.52587890625e-5f;  // 2^-16: below it the fp64 pass takes the voxel
static_assert(NLM_TW == 62 && NLM_TD == 8 && NLM_TH == 8, "a wave is a row of 62 outputs and two halo columns");

// Omega: finite and inside the modality's mask
__device__ __forceinline__ bool in_omega(float v, int mask_mode) { return in_mask(v, mask_mode) && fabsf(v) < INFINITY; }

// ---- the pseudo-residuals ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PREP_THREADS) void k_denoise_residual(const float* __restrict__ v, float* __restrict__ r,
                                                                   unsigned D, unsigned H, unsigned W, int mask_mode) {
  const unsigned gw = (W + 3) / 4, items = D * H * gw;
  const size_t sh = W, sd = (size_t)H * W;
  for (unsigned e = blockIdx.x * PREP_THREADS + threadIdx.x; e < items; e += gridDim.x * PREP_THREADS) {
    const RowItem it = row_item(e, gw, D, H);
    const size_t row = ((size_t)it.d * H + it.h) * W;
    const bool inner = it.d > 0 && it.d + 1 < D && it.h > 0 && it.h + 1 < H;
    for (unsigned u = 0; u < 4 && it.w0 + u < W; ++u) {
      const unsigned w = it.w0 + u;
      const size_t i = row + w;
      const float x = v[i];
      float out = 0.0f;
      if (inner && w > 0 && w + 1 < W && in_omega(x, mask_mode)) {
        const float n0 = v[i - sd], n1 = v[i + sd], n2 = v[i - sh], n3 = v[i + sh], n4 = v[i - 1], n5 = v[i + 1];
        if (in_omega(n0, mask_mode) && in_omega(n1, mask_mode) && in_omega(n2, mask_mode) && in_omega(n3, mask_mode) &&
            in_omega(n4, mask_mode) && in_omega(n5, mask_mode)) {
          const double s = (((((double)n0 + (double)n1) + (double)n2) + (double)n3) + (double)n4) + (double)n5;
          out = fabsf((float)((double)x - s / 6.0));
        }
      }
      r[i] = out;
    }
  }
}

// ---- the filter --------------------------------------------------------------------------------------------------------
struct NlmParams {
  const float* v;
  float* y;
  double* part;              // per workgroup: the sum of (y - v)^2 over Omega, then |Omega| as a double
  unsigned D, H, W;
  unsigned nth, ntw;         // tiles along H and W
  int mask_mode;
  float k0, k1;              // the exponent of the weight in base 2: min(k0 + k1 S, 0), S the sum of the 27 squares
  double sigma2;
};

template <int M>
struct NlmGeom {
  static constexpr int R = M + 1;                                  // the halo
  static constexpr int PD = NLM_TD + 2 * R, PH = NLM_TH + 2 * R, PW = NLM_TW + 2 * R;
  static constexpr int SH = PW, SD = PH * PW;
  static constexpr size_t BYTES = sizeof(float) * PD * PH * PW;
};
static_assert(NlmGeom<NLM_MAX_M>::BYTES <= 160 * 1024, "the largest halo fits the LDS of a compute unit");

// The voxel at LDS position `at` again, in fp64: see "Small weights" above.  inside(td, th, tw) tells whether the
// candidate at that displacement is inside the volume.
template <int M, typename Inside>
__device__ float nlm_exact(const float* lds, int at, int mask_mode, double sigma2, Inside inside) {
  using G = NlmGeom<M>;
  const float vi = lds[at];
  double amin = INFINITY, num = 0.0, den = 0.0;
#pragma nounroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma nounroll
    for (int td = -M; td <= M; ++td)
#pragma nounroll
      for (int th = -M; th <= M; ++th)
#pragma nounroll
        for (int tw = -M; tw <= M; ++tw) {
          const int to = at + td * G::SD + th * G::SH + tw;
          const float vj = lds[to];
          if ((td == 0 && th == 0 && tw == 0) || !inside(td, th, tw) || !in_omega(vj, mask_mode)) continue;
          double s = 0.0;
          for (int od = -1; od <= 1; ++od)
            for (int oh = -1; oh <= 1; ++oh)
              for (int ow = -1; ow <= 1; ++ow) {
                const int o = od * G::SD + oh * G::SH + ow;
                const double df = (double)lds[at + o] - (double)lds[to + o];
                s += df * df;
              }
          const double d2 = s / 27.0;
          if (!(d2 < (double)INFINITY)) continue;
          const double a = fmax(d2 - 2.0 * sigma2, 0.0) / (NLM_H2 * sigma2);
          if (!(exp(-a) > 0.0)) continue;
          if (pass == 0) {
            amin = fmin(amin, a);
          } else {
            const double w = exp(-(a - amin));
            den += w;
            num += w * ((double)vj - (double)vi);
          }
        }
    if (amin == (double)INFINITY) return vi;
  }
  return (float)((double)vi + num / (den + 1.0));
}

template <int M>
__global__ __launch_bounds__(NLM_THREADS) void k_denoise_nlm(NlmParams p) {
  using G = NlmGeom<M>;
  extern __shared__ float lds[];
  const unsigned tile = blockIdx.x;
  const unsigned tw_i = tile % p.ntw, th_i = (tile / p.ntw) % p.nth, td_i = tile / (p.ntw * p.nth);
  const int d0 = (int)(td_i * NLM_TD), h0 = (int)(th_i * NLM_TH), w0 = (int)(tw_i * NLM_TW);
  const int D = (int)p.D, H = (int)p.H, W = (int)p.W;

  // the tile and its halo, the edge clamp applied here
  for (int e = threadIdx.x; e < G::PD * G::PH * G::PW; e += NLM_THREADS) {
    const int xw = e % G::PW, xh = (e / G::PW) % G::PH, xd = e / (G::PW * G::PH);
    const int gd = min(max(d0 + xd - G::R, 0), D - 1), gh = min(max(h0 + xh - G::R, 0), H - 1),
              gw = min(max(w0 + xw - G::R, 0), W - 1);
    lds[e] = p.v[((size_t)gd * H + gh) * W + gw];
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gh = h0 + wave, gw = w0 + lane - 1;
  // LDS position of (d' = -1, h, w): plane R - 1, row R + wave, column R + lane - 1
  const int at0 = (G::R - 1) * G::SD + (G::R + wave) * G::SH + (G::R - 1) + lane;
  const bool mine = gh < H && lane >= 1 && lane <= NLM_TW && gw < W;      // this thread writes outputs
  double sumsq = 0.0;
  unsigned count = 0;

  if (gh < H) {                                                           // wave-uniform
    float cv[NLM_TD + 2][3];                                              // LDS[x] of the thread's three rows, all planes
#pragma unroll
    for (int dp = 0; dp < NLM_TD + 2; ++dp)
#pragma unroll
      for (int k = 0; k < 3; ++k) cv[dp][k] = lds[at0 + dp * G::SD + (k - 1) * G::SH];
    unsigned omega = 0;                                                   // bit d: output d is written and lies in Omega
#pragma unroll
    for (int d = 0; d < NLM_TD; ++d)
      if (mine && d0 + d < D && in_omega(cv[d + 1][1], p.mask_mode)) omega |= 1u << d;

    float num[NLM_TD], den[NLM_TD], wmax[NLM_TD];
    unsigned any = 0;                                                     // bit d: a candidate with a finite distance
#pragma unroll
    for (int d = 0; d < NLM_TD; ++d) { num[d] = 0.0f; den[d] = 0.0f; wmax[d] = 0.0f; }

    if (__ballot(omega != 0) != 0ull) {                                   // wave-uniform: a row of background is skipped
#pragma nounroll
      for (int td = -M; td <= M; ++td)
#pragma nounroll
        for (int th = -M; th <= M; ++th) {
          const bool row_in = (unsigned)(gh + th) < p.H;
#pragma nounroll
          for (int tw = -M; tw <= M; ++tw) {
            if (td == 0 && th == 0 && tw == 0) continue;
            const bool col_in = row_in && (unsigned)(gw + tw) < p.W;
            const float* q = lds + at0 + td * G::SD + th * G::SH + tw;
            float P0 = 0.0f, P1 = 0.0f, vj = 0.0f;
#pragma unroll
            for (int dp = 0; dp < NLM_TD + 2; ++dp) {
              const float b0 = q[dp * G::SD - G::SH], b1 = q[dp * G::SD], b2 = q[dp * G::SD + G::SH];
              const float e0 = cv[dp][0] - b0, e1 = cv[dp][1] - b1, e2 = cv[dp][2] - b2;
              const float c = __fmaf_rn(e2, e2, __fmaf_rn(e1, e1, e0 * e0));
              const float P2 = (__shfl_up(c, 1, 64) + c) + __shfl_down(c, 1, 64);
              if (dp >= 2) {
                const int d = dp - 2;                                     // the output plane; its candidate is vj
                const float S = (P0 + P1) + P2;
                const bool ok = col_in && (unsigned)(d0 + d + td) < p.D && in_omega(vj, p.mask_mode) && S < INFINITY;
                const float w = ok ? __builtin_amdgcn_exp2f(fminf(__fmaf_rn(S, p.k1, p.k0), 0.0f)) : 0.0f;
                any |= ok ? 1u << d : 0u;
                den[d] += w;
                num[d] = __fmaf_rn(w, ok ? vj - cv[d + 1][1] : 0.0f, num[d]);      // a candidate that is not finite
                wmax[d] = fmaxf(wmax[d], w);
              }
              P0 = P1;
              P1 = P2;
              vj = b1;
            }
          }
        }
    }

#pragma unroll
    for (int d = 0; d < NLM_TD; ++d) {
      if (!mine || d0 + d >= D) continue;
      const size_t i = ((size_t)(d0 + d) * H + gh) * W + gw;
      const float vi = cv[d + 1][1];
      if (!((omega >> d) & 1u)) {                                         // outside Omega: the bits as they came
        reinterpret_cast<unsigned*>(p.y)[i] = reinterpret_cast<const unsigned*>(p.v)[i];
        continue;
      }
      float out = vi;
      if ((any >> d) & 1u) {
        if (wmax[d] >= NLM_SMALL) {
          out = vi + num[d] / (den[d] + wmax[d]);
        } else {
          const int gd = d0 + d;
          out = nlm_exact<M>(lds, at0 + (d + 1) * G::SD, p.mask_mode, p.sigma2, [&](int a, int b, int c) {
            return (unsigned)(gd + a) < p.D && (unsigned)(gh + b) < p.H && (unsigned)(gw + c) < p.W;
          });
        }
      }
      p.y[i] = out;
      const double df = (double)out - (double)vi;
      sumsq += df * df;
      ++count;
    }
  }

  // the workgroup's partials: one fixed tree per wave, the waves in their order
  __shared__ double rs[NLM_WAVES];
  __shared__ unsigned rc[NLM_WAVES];
  const double s = wave_sum_all(sumsq);
  const unsigned n = wave_sum_all(count);
  if (lane == 0) { rs[wave] = s; rc[wave] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ts = rs[0];
    unsigned tn = rc[0];
    for (int k = 1; k < NLM_WAVES; ++k) { ts += rs[k]; tn += rc[k]; }
    p.part[2 * (size_t)tile] = ts;
    p.part[2 * (size_t)tile + 1] = (double)tn;
  }
}

// One workgroup: thread t adds the partials of workgroups t, t + 256, ... in that order, then the fixed trees.
__global__ __launch_bounds__(PREP_THREADS) void k_denoise_finish(const double* __restrict__ part, unsigned nblocks,
                                                                 double* __restrict__ change) {
  __shared__ double rs[PREP_WAVES][2];
  double s = 0.0, n = 0.0;
  for (unsigned b = threadIdx.x; b < nblocks; b += PREP_THREADS) { s += part[2 * (size_t)b]; n += part[2 * (size_t)b + 1]; }
  s = wave_sum_all(s);
  n = wave_sum_all(n);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { rs[wave][0] = s; rs[wave][1] = n; }
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = rs[0][threadIdx.x];
    for (int k = 1; k < PREP_WAVES; ++k) t += rs[k][threadIdx.x];
    change[threadIdx.x] = t;
  }
}

static inline size_t nlm_tiles(int D, int H, int W) {
  return (size_t)((D + NLM_TD - 1) / NLM_TD) * (size_t)((H + NLM_TH - 1) / NLM_TH) * (size_t)((W + NLM_TW - 1) / NLM_TW);
}

template <int M>
static int nlm_launch(const NlmParams& p, unsigned tiles, hipStream_t st) {
  EFFQ_HIP(raise_lds_limit<k_denoise_nlm<M>>(NlmGeom<M>::BYTES));
  hipLaunchKernelGGL(k_denoise_nlm<M>, dim3(tiles), dim3(NLM_THREADS), NlmGeom<M>::BYTES, st, p);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // namespace effq

using namespace effq;

extern "C" {

int effq_prep_denoise_residual(const float* v, int D, int H, int W, int mask_mode, float* r, void* stream) {
  EFFQ_CHECK_ARG(v && r);
  EFFQ_CHECK_ARG(prep_fits(1, D, H, W));
  EFFQ_CHECK_ARG(mask_mode == EFFQ_PREP_MASK_NONZERO || mask_mode == EFFQ_PREP_MASK_ALL);
  EFFQ_CHECK_ARG(aligned_to(v, 4) && aligned_to(r, 4));
  const size_t bytes = sizeof(float) * (size_t)D * H * W;
  const char *a = reinterpret_cast<const char*>(v), *b = reinterpret_cast<const char*>(r);
  EFFQ_CHECK_ARG(a + bytes <= b || b + bytes <= a);
  hipLaunchKernelGGL(k_denoise_residual, dim3(prep_grid((size_t)D * H * ((W + 3) / 4))), dim3(PREP_THREADS), 0,
                     as_stream(stream), v, r, (unsigned)D, (unsigned)H, (unsigned)W, mask_mode);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_prep_denoise_ws_bytes(int D, int H, int W, size_t* bytes) {
  EFFQ_CHECK_ARG(bytes != nullptr);
  EFFQ_CHECK_ARG(prep_fits(1, D, H, W));
  *bytes = nlm_tiles(D, H, W) * 2 * sizeof(double);
  return EFFQ_OK;
}

int effq_prep_denoise_nlm(const float* v, int D, int H, int W, int mask_mode, int M, double sigma2, float* y,
                          double* change, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(v && y && change && ws);
  EFFQ_CHECK_ARG(prep_fits(1, D, H, W));
  EFFQ_CHECK_ARG(mask_mode == EFFQ_PREP_MASK_NONZERO || mask_mode == EFFQ_PREP_MASK_ALL);
  EFFQ_CHECK_ARG(M >= 1 && M <= NLM_MAX_M);
  EFFQ_CHECK_ARG(sigma2 > 0.0 && sigma2 < (double)INFINITY);
  const double log2e = 1.4426950408889634;
  const float k0 = (float)(2.0 * log2e / NLM_H2), k1 = (float)(-log2e / (27.0 * NLM_H2 * sigma2));
  EFFQ_CHECK_ARG(k1 < 0.0f && k1 > -INFINITY);            // the folded constant is a normal fp32 number
  EFFQ_CHECK_ARG(aligned_to(v, 4) && aligned_to(y, 4) && aligned_to(change, 8) && aligned_to(ws, 8));
  const size_t bytes = sizeof(float) * (size_t)D * H * W;
  const char *a = reinterpret_cast<const char*>(v), *b = reinterpret_cast<const char*>(y);
  EFFQ_CHECK_ARG(a + bytes <= b || b + bytes <= a);
  const size_t tiles = nlm_tiles(D, H, W);
  EFFQ_CHECK_WS(ws_bytes, tiles * 2 * sizeof(double));
  NlmParams p;
  p.v = v; p.y = y; p.part = static_cast<double*>(ws);
  p.D = (unsigned)D; p.H = (unsigned)H; p.W = (unsigned)W;
  p.nth = (unsigned)((H + NLM_TH - 1) / NLM_TH); p.ntw = (unsigned)((W + NLM_TW - 1) / NLM_TW);
  p.mask_mode = mask_mode; p.k0 = k0; p.k1 = k1; p.sigma2 = sigma2;
  hipStream_t st = as_stream(stream);
  int rc = EFFQ_OK;
  switch (M) {
    case 1: rc = nlm_launch<1>(p, (unsigned)tiles, st); break;
    case 2: rc = nlm_launch<2>(p, (unsigned)tiles, st); break;
    case 3: rc = nlm_launch<3>(p, (unsigned)tiles, st); break;
    case 4: rc = nlm_launch<4>(p, (unsigned)tiles, st); break;
    default: rc = nlm_launch<5>(p, (unsigned)tiles, st); break;
  }
  if (rc != EFFQ_OK) return rc;
  hipLaunchKernelGGL(k_denoise_finish, dim3(1), dim3(PREP_THREADS), 0, st, p.part, (unsigned)tiles, change);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
