// Probability and uncertainty maps on the scan's grid (`predict --save_prob / --save_unc`, predict.py): the stitched
// logits of one subject, which live on the cropped box pmin : pmin + g of the working grid G, turned into C uint8
// probability planes (C, SD, SH, SW) and one uint8 uncertainty plane (SD, SH, SW) on the SOURCE grid, in one pass.
//
// Interpolated logits.  v_c is the logit of channel c at the source voxel exactly as k_seg_labels_source has it: the
// src_axis arithmetic in fp64, the inside rule and the fp32 nesting order of the eight corners are the ones of
// seg_source.h, nothing fused.  The label map and these maps are decided from the same C numbers.
//
// EFFQ_SEG_ARGMAX (class-id mode), fp32, accurate expf / logf, a true division:
//   m = max_c v_c,  d_c = v_c == m ? 0 : v_c - m,  e_c = expf(d_c),  S = e_0 + e_1 + ... (in this order),  p_c = e_c / S
//   u = (logf(S) - sum_c p_c d_c) / ln C, the entropy from the logits: the term of a channel with e_c = 0 is 0, so
//   0 * ln 0 (and 0 * -inf) never arises.  C = 1: p = 1, u = 0 (a NaN logit: NaN, stored as 0).
//   `v_c == m ? 0` changes nothing for finite values (v - v = 0) and gives the limits for infinite ones: k channels at
//   +inf share p = 1 / k, all channels at -inf share 1 / C.
// EFFQ_SEG_SIGMOID, per RAW channel (no merge, no threshold):
//   a = |v_c|, t = expf(-a):  p_c = 1 / (1 + t) for v_c >= 0 and t / (1 + t) for v_c < 0, which is 1 / (1 + exp(-v_c))
//   with one exponential that cannot overflow
//   u = max_c h(v_c), the binary entropy in bits in its softplus form, from the same a and t:
//   h = (logf(1 + t) + a t / (1 + t)) * (1 / ln 2), and h = 0 when t = 0 (a beyond about 104, and +-inf); a NaN
//   channel makes u NaN.
// Stored value: rintf(255.0f * x) as uint8 with x clamped to [0, 1], half to even; a NaN x is stored as 0.  Outside the
// box (the inside rule of seg_source.hip): sigmoid every channel 0; class-id channel 0 = 255 and the others 0, the
// background the label map writes there; u = 0.
//
// Error: with expf and logf within 3 ulp and the division within 2.5 ulp, 255 p is within 5e-4 of a
// level of the exact value of the fp32 v_c, 255 u within 1e-3; the fast intrinsics (__expf: no ulp bound over the
// range) are not used.  The exponentials are not what the pass waits for: it is gather-bound as the label kernel is.
//
// Shape: the row items of k_seg_labels_source - four consecutive w per thread, d and h worked out once per item - and
// per item one 4-byte store per plane where SW % 4 == 0 and the plane's base is 4-byte aligned (a plane starts at a
// multiple of SD SH SW, which is aligned when SW is), byte stores otherwise.  Either output may be null, not both.  No
// atomics, no reductions: equal inputs give equal bits.  Every index is 32-bit: C SD SH SW < 2^31 is checked.
#include "common.h"
#include "seg_source.h"

namespace effq {

struct ProbParams {
  const float* logits;      // (C, gd, gh, gw)
  uint8_t* probs;           // (C, SD, SH, SW) or null
  uint8_t* unc;             // (SD, SH, SW) or null
  unsigned SD, SH, SW;      // source grid
  int G[3], pmin[3], g[3];  // working grid, low corner and extent of the box
  double f[3];
  int al4p, al4u;           // every group of four of the probability planes / of the uncertainty plane lies on a 4-B boundary
};

// the stored value of x in [0, 1]: NaN -> 0
__device__ __forceinline__ uint8_t prob_level(float x) {
  if (!(x == x)) return 0;
  x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
  return (uint8_t)rintf(255.0f * x);
}

// ln C as the fp32 nearest, C = 2 .. 8 (C = 1 never divides)
template <int C>
__device__ __forceinline__ constexpr float ln_classes() {
  constexpr float t[9] = {1.0f, 1.0f, 0.693147181f, 1.09861229f, 1.38629436f, 1.60943791f, 1.79175947f, 1.94591015f,
                          2.07944154f};
  return t[C];
}

// p[c] and u of one voxel from its C interpolated logits
template <int MODE, int C>
__device__ __forceinline__ void probs_of(const float* v, float* p, float& u) {
  if constexpr (MODE == EFFQ_SEG_ARGMAX) {
    if constexpr (C == 1) {
      p[0] = v[0] == v[0] ? 1.0f : v[0];
      u = p[0] == p[0] ? 0.0f : p[0];
    } else {
      float m = v[0];
#pragma unroll
      for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
      float d[C], e[C], S = 0.0f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        d[c] = v[c] == m ? 0.0f : v[c] - m;
        e[c] = expf(d[c]);
        S = c == 0 ? e[0] : S + e[c];
      }
      float dot = 0.0f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        p[c] = e[c] / S;
        const float term = e[c] > 0.0f ? p[c] * d[c] : 0.0f;
        dot = c == 0 ? term : dot + term;
      }
      u = (logf(S) - dot) / ln_classes<C>();
    }
  } else {
    u = 0.0f;
    bool nan = false;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float a = fabsf(v[c]);
      const float t = expf(-a);
      const float one = 1.0f + t;
      p[c] = v[c] >= 0.0f ? 1.0f / one : t / one;          // a NaN v: t / one = NaN
      const float h = t > 0.0f ? (logf(one) + a * t / one) * 1.44269504f : 0.0f;
      nan = nan || !(v[c] == v[c]);
      u = fmaxf(u, h);            // a NaN v gives h = 0 here and is put back below
    }
    if (nan) u = __builtin_nanf("");
  }
}

template <int MODE, int C>
__global__ __launch_bounds__(SRC_THREADS) void k_seg_probs_source(ProbParams p) {
  const unsigned gw4 = (p.SW + 3) / 4, total = p.SD * p.SH * gw4;
  const unsigned gh = (unsigned)p.g[1], gw = (unsigned)p.g[2];
  const unsigned plane = (unsigned)p.g[0] * gh * gw;
  const size_t splane = (size_t)p.SD * p.SH * p.SW;
  for (unsigned e = blockIdx.x * SRC_THREADS + threadIdx.x; e < total; e += gridDim.x * SRC_THREADS) {
    const unsigned row = e / gw4, w0 = (e - row * gw4) * 4;
    const unsigned d = row / p.SH, h = row - d * p.SH;
    const SrcAxis ad = src_axis(d, p.f[0], p.G[0], p.pmin[0], p.g[0]);
    const SrcAxis ah = src_axis(h, p.f[1], p.G[1], p.pmin[1], p.g[1]);
    uint8_t q[C][4], qu[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const uint8_t bg = (MODE == EFFQ_SEG_ARGMAX && c == 0) ? 255 : 0;     // outside the box
#pragma unroll
      for (int u = 0; u < 4; ++u) q[c][u] = bg;
    }
    if (ad.inside && ah.inside) {
      const float* r00 = p.logits + (ad.i0 * gh + ah.i0) * gw;
      const float* r01 = p.logits + (ad.i0 * gh + ah.i1) * gw;
      const float* r10 = p.logits + (ad.i1 * gh + ah.i0) * gw;
      const float* r11 = p.logits + (ad.i1 * gh + ah.i1) * gw;
#pragma unroll
      for (unsigned u = 0; u < 4; ++u) {
        const unsigned w = min(w0 + u, p.SW - 1);
        const SrcAxis aw = src_axis(w, p.f[2], p.G[2], p.pmin[2], p.g[2]);
        if (!aw.inside) continue;
        float v[C], pr[C], un;
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = src_blend(r00, r01, r10, r11, (unsigned)c * plane, ad, ah, aw);
        probs_of<MODE, C>(v, pr, un);
#pragma unroll
        for (int c = 0; c < C; ++c) q[c][u] = prob_level(pr[c]);
        qu[u] = prob_level(un);
      }
    }
    const size_t at = (size_t)row * p.SW + w0;
    if (p.probs) {
#pragma unroll
      for (int c = 0; c < C; ++c) src_store4(p.probs + (size_t)c * splane + at, q[c], w0, p.SW, p.al4p);
    }
    if (p.unc) src_store4(p.unc + at, qu, w0, p.SW, p.al4u);
  }
}

template <int C>
static void launch_probs(int mode, dim3 g, hipStream_t st, const ProbParams& p) {
  const dim3 t(SRC_THREADS);
  if (mode == EFFQ_SEG_ARGMAX) hipLaunchKernelGGL((k_seg_probs_source<EFFQ_SEG_ARGMAX, C>), g, t, 0, st, p);
  else hipLaunchKernelGGL((k_seg_probs_source<EFFQ_SEG_SIGMOID, C>), g, t, 0, st, p);
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_seg_probs_source(const float* logits, int C, const int* box, const int* pmin, const int* grid,
                          const double* factors, const int* source, int mode, uint8_t* probs, uint8_t* unc,
                          void* stream) {
  EFFQ_CHECK_ARG(logits && box && pmin && grid && factors && source && (probs || unc));
  EFFQ_CHECK_ARG(C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID);
  EFFQ_CHECK_ARG(source_fits(probs ? C : 1, source[0], source[1], source[2]));
  EFFQ_CHECK_ARG(source_fits(1, grid[0], grid[1], grid[2]));
  EFFQ_CHECK_ARG(source_fits(C, box[0], box[1], box[2]));
  for (int a = 0; a < 3; ++a) {
    EFFQ_CHECK_ARG(0 <= pmin[a] && pmin[a] <= grid[a] - box[a]);
    EFFQ_CHECK_ARG(factors[a] > 0.0 && factors[a] <= 1e6);          // false for a NaN
  }
  EFFQ_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 3) == 0);
  ProbParams p;
  p.logits = logits; p.probs = probs; p.unc = unc;
  p.SD = source[0]; p.SH = source[1]; p.SW = source[2];
  for (int a = 0; a < 3; ++a) { p.G[a] = grid[a]; p.pmin[a] = pmin[a]; p.g[a] = box[a]; p.f[a] = factors[a]; }
  p.al4p = source[2] % 4 == 0 && (reinterpret_cast<uintptr_t>(probs) & 3) == 0;
  p.al4u = source[2] % 4 == 0 && (reinterpret_cast<uintptr_t>(unc) & 3) == 0;
  const dim3 g(source_blocks(source));
  const hipStream_t st = as_stream(stream);
  switch (C) {
    case 1: launch_probs<1>(mode, g, st, p); break;
    case 2: launch_probs<2>(mode, g, st, p); break;
    case 3: launch_probs<3>(mode, g, st, p); break;
    case 4: launch_probs<4>(mode, g, st, p); break;
    case 5: launch_probs<5>(mode, g, st, p); break;
    case 6: launch_probs<6>(mode, g, st, p); break;
    case 7: launch_probs<7>(mode, g, st, p); break;
    default: launch_probs<8>(mode, g, st, p); break;
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
