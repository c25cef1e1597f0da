// The kernels of predict --crf (crf.py, where the rule stands; restated in include/effq_hip.h): mean-field iterations of a
// locally connected conditional random field over the stitched logits, the pair weights taken from the standardised scans.
//   k_crf_table   the spatial factors w_a g_p(t) and w_s g_s(t) of every offset t of the neighbourhood, once per call; it
//                 also clears the integer `changed`;
//   k_crf_step    one iteration H' = v + sum_j k(i, j) msg(H_j), one launch each: an iteration needs every neighbour's
//                 state of the iteration before, which is a dependency across the whole grid.
//
// The state is H, never Q.  The launches ping-pong between two (C, D, H, W) buffers of the workspace (the first reads the
// logits, the last writes `out`), and the message msg(H_j) - the softmax over the C classes, or 2 sigmoid - 1 per channel -
// is formed while a voxel is staged, halo included: there is no normalisation pass and no Q array in memory.
//
// The step.  A workgroup of CRF_THREADS = 128 (two waves) owns a column of TD x TH x TW = 16 x 8 x 16 outputs, W fastest,
// and marches along D over a ring of CRF_SLOTS = 8 planes in LDS.  A plane holds the tile's footprint plus a halo of r_h
// and r_w voxels, (8 + 2 r_h) x (16 + 2 r_w) positions, and per position F = C + M floats, feature-major:
//   slot[f][ph][pw],  f < C: the message of class f,  f >= C: the intensity of modality f - C.
// A position outside the volume, or whose C + M values are not all finite, holds F zeros: it sends no message and its
// pair weight stays finite.  At the radii 3 3 3 a plane has 14 x 22 = 308 positions and the ring takes
//   8 x 308 x F x 4 B:  39 KB at F = 4 (C 3, M 1),  69 KB at F = 7 (C 3, M 4),  118 KB at F = 12 (C 8, M 4)
// of the 160 KB of a compute unit: 4, 2 and 1 workgroups, that is 8, 4 and 2 waves per compute unit.
// Output plane s needs the ring planes s .. s + 2 r_d; plane s + 2 r_d is staged at the start of step s into slot
// (s + 2 r_d) & 7, which no reader of step s - 1 or s touches while 2 r_d + 1 <= 7, so one barrier per step is enough.
// A thread owns one voxel per step: its C accumulators and its own M intensities stay in registers.  Per pair it reads the
// neighbour's M intensities and C messages from LDS (consecutive lanes, consecutive addresses) and forms
//   k = fma(w_a g_p, exp2(ki * sum_m (x_m(i) - x_m(j))^2), w_s g_s),   ki = -log2(e) / (2 theta_i^2) folded on the host,
// __builtin_amdgcn_exp2f being the v_exp_f32 instruction (1 ulp).  The two spatial factors of the offset are uniform over
// the workgroup and come from the table through scalar loads.  At r_w = 3 (a W spacing of at most 2 max(theta_p, theta_s) / 3 mm: 2 mm
// with the defaults, so not the slice axis of thick-slice scans) the seven pairs of a row are unrolled (k_crf_step<C,
// true>) so that their LDS reads are in flight together: with one or two waves per SIMD there is little else to hide them
// behind.  Every other r_w takes the rolled loop (k_crf_step<C, false>).  The order of the sums is the same in both forms.  The weights differ per pair, so
// there is no matrix product to hand to the matrix cores.
//
// A voxel whose C logits and M intensities are not all finite keeps H = v, bit for bit.  `changed` counts the voxels whose
// decision differs between v and the last H: a thread counts its own voxels along the march, the counts are summed per
// wave by lane exchanges (wave_sum_all), and the last launch issues one integer atomic per workgroup.  No floating-point atomic; the order of every sum is fixed by the offsets: equal inputs give equal bits.
#include <math.h>
#include "common.h"
#include "prep_rows.h"

namespace effq {

constexpr int CRF_TD = EFFQ_SEG_CRF_TILE_D, CRF_TH = EFFQ_SEG_CRF_TILE_H, CRF_TW = EFFQ_SEG_CRF_TILE_W;
constexpr int CRF_THREADS = CRF_TH * CRF_TW, CRF_WAVES = CRF_THREADS / 64;
constexpr int CRF_R = EFFQ_SEG_CRF_MAX_RADIUS, CRF_MAX_C = EFFQ_SEG_CRF_MAX_CLASSES, CRF_MAX_M = EFFQ_SEG_CRF_MAX_MODALITIES;
constexpr int CRF_SLOTS = 8;
constexpr int CRF_TAB = (2 * CRF_R + 1) * (2 * CRF_R + 1) * (2 * CRF_R + 1);
constexpr size_t CRF_TAB_BYTES = 4096;                  // 2 floats per offset, rounded up: the buffers stay aligned
constexpr float CRF_LOG2E = 1.44269504088896340736f;
static_assert(CRF_THREADS % 64 == 0 && 2 * CRF_R + 1 < CRF_SLOTS, "whole waves; the ring holds one plane more than is read");
static_assert(2 * sizeof(float) * CRF_TAB <= CRF_TAB_BYTES, "the table fits its part of the workspace");
static_assert(sizeof(float) * CRF_SLOTS * (CRF_MAX_C + CRF_MAX_M) * (CRF_TH + 2 * CRF_R) * (CRF_TW + 2 * CRF_R) + 64 <=
              160 * 1024, "the largest ring fits the LDS of a compute unit");

__device__ __forceinline__ bool crf_finite(float v) { return fabsf(v) < INFINITY; }

// ---- the spatial factors -----------------------------------------------------------------------------------------------
// entry t = ((dd + rd) (2 rh + 1) + dh + rh) (2 rw + 1) + dw + rw:  tab[2 t] = ap exp(cp e),  tab[2 t + 1] = as exp(cs e)
// with e = d2 - the least d2 of the neighbourhood, ap = w_a / Z_p, cp = -1 / (2 theta_p^2) and the same for the smoothness
// kernel, all fp64, rounded once.  Taking the least d2 out of the exponent and out of Z leaves g = exp(cp d2) / Z what it
// is and keeps Z >= 1 however small a width is against the spacing.
__global__ __launch_bounds__(CRF_TAB + 41) void k_crf_table(float* __restrict__ tab, unsigned* __restrict__ changed, int rd,
                                                            int rh, int rw, double sd, double sh, double sw, double d2min,
                                                            double ap, double cp, double as, double cs) {
  const int t = threadIdx.x, nh = 2 * rh + 1, nw = 2 * rw + 1;
  if (t == 0) *changed = 0u;
  if (t >= (2 * rd + 1) * nh * nw) return;
  const double dd = sd * (t / (nh * nw) - rd), dh = sh * ((t / nw) % nh - rh), dw = sw * (t % nw - rw);
  const double e = fmax(dd * dd + dh * dh + dw * dw - d2min, 0.0);
  tab[2 * t] = (float)(ap * exp(cp * e));
  tab[2 * t + 1] = (float)(as * exp(cs * e));
}

// ---- one iteration -----------------------------------------------------------------------------------------------------
struct CrfStep {
  const float* src;          // H of the iteration before (C, D, H, W); the logits in the first launch
  const float* v;            // the logits
  const float* x;            // the images (M, D, H, W)
  float* dst;
  const float* tab;
  unsigned* changed;         // the last launch counts; null before
  int D, H, W, M;
  int rd, rh, rw;
  unsigned nth, ntw;         // tiles along H and W
  int mode;
  float ki;                  // -log2(e) / (2 theta_i^2)
  float thresh;
};

template <int C, bool FULLW>
__global__ __launch_bounds__(CRF_THREADS) void k_crf_step(CrfStep p) {
  extern __shared__ float lds[];
  __shared__ unsigned wave_count[CRF_WAVES];
  const int D = p.D, H = p.H, W = p.W, M = p.M;
  const int PW = CRF_TW + 2 * p.rw, PP = (CRF_TH + 2 * p.rh) * PW, slot_stride = (C + M) * PP;
  const unsigned tile = blockIdx.x;
  const int w0 = (int)(tile % p.ntw) * CRF_TW, h0 = (int)((tile / p.ntw) % p.nth) * CRF_TH,
            d0 = (int)(tile / (p.ntw * p.nth)) * CRF_TD;
  const int nd = min(CRF_TD, D - d0);
  const size_t plane = (size_t)H * W, vol = plane * D;

  // ring plane n = the volume's plane d0 - rd + n, into slot n & 7; the message is formed here
  auto stage = [&](int n) {
    const int gd = d0 - p.rd + n;
    float* s = lds + (n & (CRF_SLOTS - 1)) * slot_stride;
    for (int e = threadIdx.x; e < PP; e += CRF_THREADS) {
      const int gh = h0 - p.rh + e / PW, gw = w0 - p.rw + e % PW;
      float q[C], xv[CRF_MAX_M];
      bool ok = (unsigned)gd < (unsigned)D && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W;
      if (ok) {
        const size_t i = (size_t)gd * plane + (size_t)gh * W + gw;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          q[c] = p.src[c * vol + i];
          ok = ok && crf_finite(q[c]);
        }
#pragma unroll
        for (int m = 0; m < CRF_MAX_M; ++m)
          if (m < M) {
            xv[m] = p.x[m * vol + i];
            ok = ok && crf_finite(xv[m]);
          }
      }
      if (ok) {
        if (p.mode == EFFQ_SEG_ARGMAX) {
          float mx = q[0], sum = 0.0f;
#pragma unroll
          for (int c = 1; c < C; ++c) mx = fmaxf(mx, q[c]);
#pragma unroll
          for (int c = 0; c < C; ++c) {
            q[c] = __builtin_amdgcn_exp2f((q[c] - mx) * CRF_LOG2E);
            sum += q[c];
          }
#pragma unroll
          for (int c = 0; c < C; ++c) q[c] = q[c] / sum;
        } else {
#pragma unroll
          for (int c = 0; c < C; ++c) q[c] = 2.0f / (1.0f + __builtin_amdgcn_exp2f(-q[c] * CRF_LOG2E)) - 1.0f;
        }
      }
#pragma unroll
      for (int c = 0; c < C; ++c) s[c * PP + e] = ok ? q[c] : 0.0f;
#pragma unroll
      for (int m = 0; m < CRF_MAX_M; ++m)
        if (m < M) s[(C + m) * PP + e] = ok ? xv[m] : 0.0f;
    }
  };

  const int lh = threadIdx.x / CRF_TW, lw = threadIdx.x % CRF_TW;
  const int gh = h0 + lh, gw = w0 + lw;
  const bool mine = gh < H && gw < W;
  const int at = (lh + p.rh) * PW + lw + p.rw;            // the thread's position in a plane
  const int nh = 2 * p.rh + 1, nw = 2 * p.rw + 1;
  unsigned count = 0;

  for (int n = 0; n < 2 * p.rd; ++n) stage(n);
  for (int s = 0; s < nd; ++s) {
    stage(s + 2 * p.rd);
    __syncthreads();
    if (!mine) continue;
    const size_t i = (size_t)(d0 + s) * plane + (size_t)gh * W + gw;
    float vi[C], xi[CRF_MAX_M], acc[C];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      vi[c] = p.v[c * vol + i];
      acc[c] = 0.0f;
      ok = ok && crf_finite(vi[c]);
    }
#pragma unroll
    for (int m = 0; m < CRF_MAX_M; ++m) {
      xi[m] = m < M ? p.x[m * vol + i] : 0.0f;
      ok = ok && crf_finite(xi[m]);
    }
    if (!ok) {                                            // sends nothing, receives nothing: the bits as they came
#pragma unroll
      for (int c = 0; c < C; ++c)
        reinterpret_cast<unsigned*>(p.dst)[c * vol + i] = reinterpret_cast<const unsigned*>(p.v)[c * vol + i];
      continue;
    }
#pragma nounroll
    for (int dd = -p.rd; dd <= p.rd; ++dd) {
      const float* sl = lds + ((s + p.rd + dd) & (CRF_SLOTS - 1)) * slot_stride + at;
#pragma nounroll
      for (int dh = -p.rh; dh <= p.rh; ++dh) {
        auto pair = [&](int dw) {
          if (dd == 0 && dh == 0 && dw == 0) return;
          const int t = ((dd + p.rd) * nh + dh + p.rh) * nw + dw + p.rw;
          const float ga = p.tab[2 * t], gs = p.tab[2 * t + 1];
          const float* q = sl + dh * PW + dw;
          float a = 0.0f;
#pragma unroll
          for (int m = 0; m < CRF_MAX_M; ++m)
            if (m < M) {
              const float df = xi[m] - q[(C + m) * PP];
              a = __fmaf_rn(df, df, a);
            }
          const float k = __fmaf_rn(ga, __builtin_amdgcn_exp2f(a * p.ki), gs);
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] = __fmaf_rn(k, q[c * PP], acc[c]);
        };
        if constexpr (FULLW) {                            // r_w = 3: the seven pairs of a row unrolled, their reads in flight
#pragma unroll
          for (int dw = -CRF_R; dw <= CRF_R; ++dw) pair(dw);
        } else {
#pragma nounroll
          for (int dw = -p.rw; dw <= p.rw; ++dw) pair(dw);
        }
      }
    }
    float h[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      h[c] = vi[c] + acc[c];
      p.dst[c * vol + i] = h[c];
    }
    if (p.changed != nullptr) {
      bool differs = false;
      if (p.mode == EFFQ_SEG_ARGMAX) {                    // the first maximum wins
        int bv = 0, bh = 0;
#pragma unroll
        for (int c = 1; c < C; ++c) {
          if (vi[c] > vi[bv]) bv = c;
          if (h[c] > h[bh]) bh = c;
        }
        differs = bv != bh;
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) differs = differs || ((vi[c] >= p.thresh) != (h[c] >= p.thresh));
      }
      count += differs ? 1u : 0u;
    }
  }

  if (p.changed != nullptr) {                             // uniform over the grid
    const unsigned n = wave_sum_all(count);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned total = 0;
      for (int k = 0; k < CRF_WAVES; ++k) total += wave_count[k];
      if (total) atomicAdd(p.changed, total);
    }
  }
}

static inline size_t crf_lds_bytes(int C, int M, int rh, int rw) {
  return sizeof(float) * CRF_SLOTS * (size_t)(C + M) * (CRF_TH + 2 * rh) * (CRF_TW + 2 * rw);
}

template <int C>
static int crf_launch(const CrfStep& p, unsigned tiles, hipStream_t st) {
  const size_t bytes = crf_lds_bytes(C, p.M, p.rh, p.rw);
  if (p.rw == CRF_R) {
    EFFQ_HIP((raise_lds_limit<k_crf_step<C, true>>(bytes)));
    hipLaunchKernelGGL((k_crf_step<C, true>), dim3(tiles), dim3(CRF_THREADS), bytes, st, p);
  } else {
    EFFQ_HIP((raise_lds_limit<k_crf_step<C, false>>(bytes)));
    hipLaunchKernelGGL((k_crf_step<C, false>), dim3(tiles), dim3(CRF_THREADS), bytes, st, p);
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

static int crf_step(int C, const CrfStep& p, unsigned tiles, hipStream_t st) {
  switch (C) {
    case 1: return crf_launch<1>(p, tiles, st);
    case 2: return crf_launch<2>(p, tiles, st);
    case 3: return crf_launch<3>(p, tiles, st);
    case 4: return crf_launch<4>(p, tiles, st);
    case 5: return crf_launch<5>(p, tiles, st);
    case 6: return crf_launch<6>(p, tiles, st);
    case 7: return crf_launch<7>(p, tiles, st);
    default: return crf_launch<8>(p, tiles, st);
  }
}

// whether n planes of D x H x W voxels are a volume the kernels index: every extent at least 1, n D H W < 2^31
static inline bool crf_fits(int n, int D, int H, int W) {
  if (n < 1 || D < 1 || H < 1 || W < 1) return false;
  const unsigned long long lim = 2147483647ull;
  unsigned long long e = (unsigned long long)D * (unsigned long long)H;
  if (e > lim) return false;
  e *= (unsigned long long)W;
  if (e > lim) return false;
  return e * (unsigned long long)n <= lim;
}

static inline bool crf_apart(const void* a, size_t na, const void* b, size_t nb) {
  const char *x = static_cast<const char*>(a), *y = static_cast<const char*>(b);
  return x + na <= y || y + nb <= x;
}

static inline bool crf_positive(double v) { return v > 0.0 && v < (double)INFINITY; }
static inline bool crf_width(double v) { return v >= EFFQ_SEG_CRF_THETA_MIN && v <= EFFQ_SEG_CRF_THETA_MAX; }

}  // namespace effq

using namespace effq;

extern "C" {

int effq_seg_crf_ws_bytes(int C, int D, int H, int W, size_t* need) {
  EFFQ_CHECK_ARG(need != nullptr);
  EFFQ_CHECK_ARG(C >= 1 && C <= CRF_MAX_C);
  EFFQ_CHECK_ARG(crf_fits(C, D, H, W));
  *need = CRF_TAB_BYTES + 2 * sizeof(float) * (size_t)C * D * H * W;
  return EFFQ_OK;
}

int effq_seg_crf(const float* logits, int C, const float* images, int M, int D, int H, int W, double s_d, double s_h,
                 double s_w, int mode, double w_a, double w_s, double theta_p, double theta_i, double theta_s, int iters,
                 float thresh_logit, float* out, unsigned* changed, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(logits && images && out && changed && ws);
  EFFQ_CHECK_ARG(mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID);
  EFFQ_CHECK_ARG(C >= (mode == EFFQ_SEG_ARGMAX ? 2 : 1) && C <= CRF_MAX_C);
  EFFQ_CHECK_ARG(M >= 1 && M <= CRF_MAX_M);
  EFFQ_CHECK_ARG(crf_fits(C > M ? C : M, D, H, W));
  EFFQ_CHECK_ARG(crf_positive(s_d) && crf_positive(s_h) && crf_positive(s_w));
  EFFQ_CHECK_ARG(w_a >= 0.0 && w_s >= 0.0 && w_a + w_s <= (double)EFFQ_SEG_CRF_MAX_WEIGHT);
  EFFQ_CHECK_ARG(crf_width(theta_p) && crf_width(theta_i) && crf_width(theta_s));
  EFFQ_CHECK_ARG(iters >= 1 && iters <= EFFQ_SEG_CRF_MAX_ITERS);
  EFFQ_CHECK_ARG(fabsf(thresh_logit) < INFINITY);
  const float ki = (float)(-1.4426950408889634 / (2.0 * theta_i * theta_i));
  EFFQ_CHECK_ARG(ki < -1.17549435e-38f && ki > -INFINITY);        // a normal fp32 number for every width in the range
  // the radii: min(3, floor(2 max(theta_p, theta_s) / s_a)); an axis with radius 0 is not linked
  const double reach = 2.0 * (theta_p > theta_s ? theta_p : theta_s), sp[3] = {s_d, s_h, s_w};
  int r[3];
  for (int a = 0; a < 3; ++a) {
    const double q = floor(reach / sp[a]);
    r[a] = q >= (double)CRF_R ? CRF_R : (int)q;
  }
  EFFQ_CHECK_ARG(r[0] + r[1] + r[2] > 0);
  // Z of both kernels over the whole neighbourhood, borders notwithstanding
  const double cp = -1.0 / (2.0 * theta_p * theta_p), cs = -1.0 / (2.0 * theta_s * theta_s);
  double zp = 0.0, zs = 0.0, d2min = INFINITY;
  for (int pass = 0; pass < 2; ++pass)                    // the least d2, then Z relative to it
    for (int dd = -r[0]; dd <= r[0]; ++dd)
      for (int dh = -r[1]; dh <= r[1]; ++dh)
        for (int dw = -r[2]; dw <= r[2]; ++dw) {
          if (dd == 0 && dh == 0 && dw == 0) continue;
          const double d2 = (s_d * dd) * (s_d * dd) + (s_h * dh) * (s_h * dh) + (s_w * dw) * (s_w * dw);
          if (pass == 0) {
            d2min = d2 < d2min ? d2 : d2min;
          } else {
            zp += exp(cp * (d2 - d2min));
            zs += exp(cs * (d2 - d2min));
          }
        }
  EFFQ_CHECK_ARG(crf_positive(d2min) && zp >= 1.0 && zs >= 1.0 && zp < (double)INFINITY && zs < (double)INFINITY);
  EFFQ_CHECK_ARG(aligned_to(logits, 4) && aligned_to(images, 4) && aligned_to(out, 4) && aligned_to(changed, 4) &&
                 aligned_to(ws, 4));
  const size_t vol = (size_t)D * H * W, bytes = sizeof(float) * (size_t)C * vol;
  EFFQ_CHECK_ARG(crf_apart(out, bytes, logits, bytes) && crf_apart(out, bytes, images, sizeof(float) * (size_t)M * vol));
  EFFQ_CHECK_ARG(crf_apart(changed, sizeof(unsigned), out, bytes) && crf_apart(changed, sizeof(unsigned), logits, bytes) &&
                 crf_apart(changed, sizeof(unsigned), images, sizeof(float) * (size_t)M * vol));
  EFFQ_CHECK_WS(ws_bytes, CRF_TAB_BYTES + 2 * bytes);
  EFFQ_CHECK_ARG(crf_apart(ws, CRF_TAB_BYTES + 2 * bytes, out, bytes) && crf_apart(ws, CRF_TAB_BYTES + 2 * bytes, logits, bytes) &&
                 crf_apart(ws, CRF_TAB_BYTES + 2 * bytes, images, sizeof(float) * (size_t)M * vol) &&
                 crf_apart(ws, CRF_TAB_BYTES + 2 * bytes, changed, sizeof(unsigned)));

  hipStream_t st = as_stream(stream);
  float* tab = static_cast<float*>(ws);
  float* buf[2] = {reinterpret_cast<float*>(static_cast<char*>(ws) + CRF_TAB_BYTES), nullptr};
  buf[1] = buf[0] + (size_t)C * vol;
  hipLaunchKernelGGL(k_crf_table, dim3(1), dim3(CRF_TAB + 41), 0, st, tab, changed, r[0], r[1], r[2], s_d, s_h, s_w,
                     d2min, w_a / zp, cp, w_s / zs, cs);
  EFFQ_LAUNCH_CHECK();
  CrfStep p;
  p.v = logits; p.x = images; p.tab = tab;
  p.D = D; p.H = H; p.W = W; p.M = M;
  p.rd = r[0]; p.rh = r[1]; p.rw = r[2];
  p.nth = (unsigned)((H + CRF_TH - 1) / CRF_TH); p.ntw = (unsigned)((W + CRF_TW - 1) / CRF_TW);
  p.mode = mode; p.ki = ki; p.thresh = thresh_logit;
  const size_t tiles = (size_t)((D + CRF_TD - 1) / CRF_TD) * p.nth * p.ntw;
  for (int t = 0; t < iters; ++t) {
    p.src = t == 0 ? logits : buf[(t - 1) & 1];
    p.dst = t == iters - 1 ? out : buf[t & 1];
    p.changed = t == iters - 1 ? changed : nullptr;
    const int rc = crf_step(C, p, (unsigned)tiles, st);
    if (rc != EFFQ_OK) return rc;
  }
  return EFFQ_OK;
}

}  // extern "C"
