// Validation of a segmentation network on whole volumes (evaluate.validate_seg), after window.hip has stitched the
// logits: the per-class confusion counts of the stitched logits against the label, the label maps written for the viewer
// (--save_nii), and the counts of a label map against the label (effq_label_tallies, the score of a map cleaned by
// --post).  All three stream HBM once and do no arithmetic to speak of.
//
// Tallies: wave reductions into per-block partials, summed in block order by a second launch; integer counts only.
#include "common.h"
#include "seg_decide.h"
#include "seg_window.h"      // grid_for

namespace effq {

// ---- tallies ------------------------------------------------------------------------------------------------------
// per class three counters: true positives, predicted positives, labelled positives (FP, FN and TN follow from them)
constexpr int TALLY_THREADS = 256;
constexpr int TALLY_WAVES = TALLY_THREADS / 64;
constexpr int TALLY_MAX_BLOCKS = 1024;
constexpr int TALLY_NCNT = 3 * EFFQ_SEG_TALLIES_MAX_CLASSES;
static_assert((size_t)TALLY_MAX_BLOCKS * TALLY_NCNT * sizeof(uint32_t) <= EFFQ_SEG_TALLIES_WS_BYTES, "workspace");

struct TallyParams {
  const float* logits;    // (C, S)
  const uint8_t* label;   // (S) class ids for argmax, (C, S) 0/1 for multi-label
  uint32_t* partial;      // (gridDim.x, 3 * C)
  long long S;
  int C, mode, fuse;
  float thresh;
};

// C classes known at compile time: every per-class loop unrolls and each thread keeps 3 C counters
template <int MODE, int VEC, int C>
__global__ __launch_bounds__(TALLY_THREADS) void k_seg_tallies(TallyParams p) {
  uint32_t cnt[3 * C];
#pragma unroll
  for (int q = 0; q < 3 * C; ++q) cnt[q] = 0;
  const long long groups = p.S / VEC;
  const long long lab_stride = MODE == EFFQ_SEG_ARGMAX ? 0 : p.S;
  for (long long g = (long long)blockIdx.x * TALLY_THREADS + threadIdx.x; g < groups;
       g += (long long)gridDim.x * TALLY_THREADS) {
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
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      uint32_t pred, gt;
      decide<MODE, C>(v[u], lab[u], p.fuse, p.thresh, pred, gt);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        cnt[3 * c + 0] += (pred >> c) & (gt >> c) & 1u;
        cnt[3 * c + 1] += (pred >> c) & 1u;
        cnt[3 * c + 2] += (gt >> c) & 1u;
      }
    }
  }
  __shared__ uint32_t red[TALLY_WAVES][3 * C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 3 * C; ++q) {
    const uint32_t s = wave_sum_all(cnt[q]);
    if (lane == 0) red[wave][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < 3 * C) {
    uint32_t s = 0;
    for (int w = 0; w < TALLY_WAVES; ++w) s += red[w][threadIdx.x];
    p.partial[(size_t)blockIdx.x * 3 * C + threadIdx.x] = s;
  }
}

// one thread per counter adds the partials in block order; out (C, 4) = TP, FP, FN, TN
__global__ __launch_bounds__(64) void k_seg_tallies_final(const uint32_t* __restrict__ partial, int nblocks, int C,
                                                          long long S, long long* __restrict__ out) {
  __shared__ long long tot[TALLY_NCNT];
  const int q = threadIdx.x;
  if (q < 3 * C) {
    long long s = 0;
    for (int b = 0; b < nblocks; ++b) s += partial[(size_t)b * 3 * C + q];
    tot[q] = s;
  }
  __syncthreads();
  if (q < C) {
    const long long tp = tot[3 * q], pp = tot[3 * q + 1], lp = tot[3 * q + 2];
    out[4 * q + 0] = tp;
    out[4 * q + 1] = pp - tp;
    out[4 * q + 2] = lp - tp;
    out[4 * q + 3] = S - pp - lp + tp;
  }
}

// ---- tallies of a label map -------------------------------------------------------------------------------------------
// effq_label_tallies: the counters of k_seg_tallies for a uint8 label map instead of logits.  The class bits of a value
// come from a 256-entry table (kept in LDS); the truth is a map read through the same table, or C 0/1 planes.  VEC 4: one
// 4-B load per thread, map and plane; the last S % 4 voxels are counted one by one by the first threads of the grid.
constexpr int LTALLY_MAX_BLOCKS = 512;
static_assert(LTALLY_MAX_BLOCKS <= TALLY_MAX_BLOCKS, "the partials fit the tallies' workspace");

struct LabelLut {
  uint16_t v[256];
};

struct LabelTallyParams {
  const uint8_t* pred;    // (S)
  const uint8_t* truth;   // (S) label values, or (C, S) 0/1 planes
  uint32_t* partial;      // (gridDim.x, 3 * C)
  long long S;
};

template <int VEC, bool PLANES, int C>
__global__ __launch_bounds__(TALLY_THREADS) void k_label_tallies(LabelTallyParams p, LabelLut lut) {
  __shared__ uint16_t s_lut[256];
  for (int k = threadIdx.x; k < 256; k += TALLY_THREADS) s_lut[k] = lut.v[k];
  __syncthreads();
  uint32_t cnt[3 * C];
#pragma unroll
  for (int q = 0; q < 3 * C; ++q) cnt[q] = 0;
  auto tally = [&](uint32_t pred, uint32_t gt) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      cnt[3 * c + 0] += (pred >> c) & (gt >> c) & 1u;
      cnt[3 * c + 1] += (pred >> c) & 1u;
      cnt[3 * c + 2] += (gt >> c) & 1u;
    }
  };
  auto truth_bits = [&](long long v) -> uint32_t {
    if constexpr (!PLANES) {
      return s_lut[p.truth[v]];
    } else {
      uint32_t gt = 0;
#pragma unroll
      for (int c = 0; c < C; ++c) gt |= (p.truth[c * p.S + v] != 0 ? 1u : 0u) << c;
      return gt;
    }
  };
  const long long groups = p.S / VEC;
  const long long tid = (long long)blockIdx.x * TALLY_THREADS + threadIdx.x;
  for (long long g = tid; g < groups; g += (long long)gridDim.x * TALLY_THREADS) {
    if constexpr (VEC == 4) {
      const uchar4 m = *reinterpret_cast<const uchar4*>(p.pred + g * 4);
      const uint32_t pr[4] = {s_lut[m.x], s_lut[m.y], s_lut[m.z], s_lut[m.w]};
      uint32_t gt[4] = {0, 0, 0, 0};
      if constexpr (!PLANES) {
        const uchar4 t = *reinterpret_cast<const uchar4*>(p.truth + g * 4);
        gt[0] = s_lut[t.x]; gt[1] = s_lut[t.y]; gt[2] = s_lut[t.z]; gt[3] = s_lut[t.w];
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const uchar4 t = *reinterpret_cast<const uchar4*>(p.truth + c * p.S + g * 4);
          gt[0] |= (t.x != 0 ? 1u : 0u) << c; gt[1] |= (t.y != 0 ? 1u : 0u) << c;
          gt[2] |= (t.z != 0 ? 1u : 0u) << c; gt[3] |= (t.w != 0 ? 1u : 0u) << c;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) tally(pr[u], gt[u]);
    } else {
      tally(s_lut[p.pred[g]], truth_bits(g));
    }
  }
  if (VEC == 4 && tid < p.S - groups * 4) {          // the tail
    const long long v = groups * 4 + tid;
    tally(s_lut[p.pred[v]], truth_bits(v));
  }
  __shared__ uint32_t red[TALLY_WAVES][3 * C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 3 * C; ++q) {
    const uint32_t s = wave_sum_all(cnt[q]);
    if (lane == 0) red[wave][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < 3 * C) {
    uint32_t s = 0;
    for (int w = 0; w < TALLY_WAVES; ++w) s += red[w][threadIdx.x];
    p.partial[(size_t)blockIdx.x * 3 * C + threadIdx.x] = s;
  }
}

template <int C>
static void launch_label_tallies(bool planes, bool v4, dim3 g, hipStream_t st, const LabelTallyParams& p,
                                 const LabelLut& lut) {
  const dim3 b(TALLY_THREADS);
  if (planes) {
    if (v4) hipLaunchKernelGGL((k_label_tallies<4, true, C>), g, b, 0, st, p, lut);
    else hipLaunchKernelGGL((k_label_tallies<1, true, C>), g, b, 0, st, p, lut);
  } else {
    if (v4) hipLaunchKernelGGL((k_label_tallies<4, false, C>), g, b, 0, st, p, lut);
    else hipLaunchKernelGGL((k_label_tallies<1, false, C>), g, b, 0, st, p, lut);
  }
}

// ---- label maps ---------------------------------------------------------------------------------------------------
// The decisions of decide<MODE, C> (the tallies' own, so the maps and the counts cannot disagree) turned into a label
// per voxel, or into C 0/1 planes.  One thread per VEC voxels, 16-B logit loads per channel, one store per thread and
// plane; no reductions, no atomics.
constexpr int LABEL_THREADS = 256;
constexpr int LABEL_MAX_BLOCKS = 2048;   // per case (gridDim.y = N); grid-stride beyond

struct LabelParams {
  const float* logits;   // (N, C, S)
  void* out;             // (N, S) uint8 / uint16, or (N, C, S) uint8 for EFFQ_SEG_LABEL_PLANES
  long long S;
  int fuse;
  float thresh;
};

template <int MODE, int RULE, int VEC, int C, typename T>
__global__ __launch_bounds__(LABEL_THREADS) void k_seg_labels(LabelParams p) {
  const long long groups = p.S / VEC;
  const size_t n = blockIdx.y;
  const float* x = p.logits + n * C * p.S;
  const uint8_t nolab[C] = {};                        // decide() wants a label; its gt bits are not used
  for (long long g = (long long)blockIdx.x * LABEL_THREADS + threadIdx.x; g < groups;
       g += (long long)gridDim.x * LABEL_THREADS) {
    float v[VEC][C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if constexpr (VEC == 4) {
        const float4 f = *reinterpret_cast<const float4*>(x + c * p.S + g * 4);
        v[0][c] = f.x; v[1][c] = f.y; v[2][c] = f.z; v[3][c] = f.w;
      } else {
        v[0][c] = x[c * p.S + g];
      }
    }
    uint32_t pred[VEC];
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      uint32_t gt;
      decide<MODE, C>(v[u], nolab, p.fuse, p.thresh, pred[u], gt);
    }
    if constexpr (RULE == EFFQ_SEG_LABEL_PLANES) {
      uint8_t* o = static_cast<uint8_t*>(p.out) + n * C * p.S;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        if constexpr (VEC == 4) {
          const uchar4 b = make_uchar4((pred[0] >> c) & 1u, (pred[1] >> c) & 1u, (pred[2] >> c) & 1u,
                                       (pred[3] >> c) & 1u);
          *reinterpret_cast<uchar4*>(o + c * p.S + g * 4) = b;
        } else {
          o[c * p.S + g] = (pred[0] >> c) & 1u;
        }
      }
    } else {
      T* o = static_cast<T*>(p.out) + n * p.S;
      if constexpr (VEC == 4) {
        const uint32_t l0 = label_of<RULE, C>(pred[0]), l1 = label_of<RULE, C>(pred[1]);
        const uint32_t l2 = label_of<RULE, C>(pred[2]), l3 = label_of<RULE, C>(pred[3]);
        if constexpr (sizeof(T) == 1)
          *reinterpret_cast<uchar4*>(o + g * 4) = make_uchar4(l0, l1, l2, l3);
        else
          *reinterpret_cast<ushort4*>(o + g * 4) = make_ushort4(l0, l1, l2, l3);
      } else {
        o[g] = (T)label_of<RULE, C>(pred[0]);
      }
    }
  }
}

template <int RULE, int C, typename T>
static void launch_labels_t(bool v4, dim3 g, hipStream_t st, const LabelParams& p) {
  constexpr int MODE = RULE == EFFQ_SEG_LABEL_ARGMAX ? EFFQ_SEG_ARGMAX : EFFQ_SEG_SIGMOID;
  if (v4) hipLaunchKernelGGL((k_seg_labels<MODE, RULE, 4, C, T>), g, dim3(LABEL_THREADS), 0, st, p);
  else hipLaunchKernelGGL((k_seg_labels<MODE, RULE, 1, C, T>), g, dim3(LABEL_THREADS), 0, st, p);
}

template <int C>
static void launch_labels(int rule, bool u16, bool v4, dim3 g, hipStream_t st, const LabelParams& p) {
  switch (rule) {
    case EFFQ_SEG_LABEL_ARGMAX:
      if (u16) launch_labels_t<EFFQ_SEG_LABEL_ARGMAX, C, uint16_t>(v4, g, st, p);
      else launch_labels_t<EFFQ_SEG_LABEL_ARGMAX, C, uint8_t>(v4, g, st, p);
      break;
    case EFFQ_SEG_LABEL_BRATS:
      if (u16) launch_labels_t<EFFQ_SEG_LABEL_BRATS, C, uint16_t>(v4, g, st, p);
      else launch_labels_t<EFFQ_SEG_LABEL_BRATS, C, uint8_t>(v4, g, st, p);
      break;
    case EFFQ_SEG_LABEL_RANK:
      if (u16) launch_labels_t<EFFQ_SEG_LABEL_RANK, C, uint16_t>(v4, g, st, p);
      else launch_labels_t<EFFQ_SEG_LABEL_RANK, C, uint8_t>(v4, g, st, p);
      break;
    default:
      launch_labels_t<EFFQ_SEG_LABEL_PLANES, C, uint8_t>(v4, g, st, p);
      break;
  }
}

template <int C>
static void launch_tallies(int mode, bool v4, dim3 g, dim3 b, hipStream_t st, const TallyParams& p) {
  if (mode == EFFQ_SEG_ARGMAX) {
    if (v4) hipLaunchKernelGGL((k_seg_tallies<EFFQ_SEG_ARGMAX, 4, C>), g, b, 0, st, p);
    else hipLaunchKernelGGL((k_seg_tallies<EFFQ_SEG_ARGMAX, 1, C>), g, b, 0, st, p);
  } else {
    if (v4) hipLaunchKernelGGL((k_seg_tallies<EFFQ_SEG_SIGMOID, 4, C>), g, b, 0, st, p);
    else hipLaunchKernelGGL((k_seg_tallies<EFFQ_SEG_SIGMOID, 1, C>), g, b, 0, st, p);
  }
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_seg_tallies(const float* logits, const uint8_t* label, int C, long long S, int mode, int fuse, float thresh,
                     long long* counts, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(logits && label && counts && ws && S > 0 && C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID);
  EFFQ_CHECK_ARG(fuse == EFFQ_SEG_FUSE_NONE || fuse == EFFQ_SEG_FUSE_AGG || fuse == EFFQ_SEG_FUSE_CON);
  EFFQ_CHECK_ARG(ws_bytes >= EFFQ_SEG_TALLIES_WS_BYTES);
  TallyParams p;
  p.logits = logits; p.label = label; p.partial = static_cast<uint32_t*>(ws);
  p.S = S; p.C = C; p.mode = mode; p.fuse = fuse; p.thresh = thresh;
  const bool v4 = S % 4 == 0 && ((reinterpret_cast<uintptr_t>(logits) & 15) | (reinterpret_cast<uintptr_t>(label) & 3)) == 0;
  const unsigned nb = grid_for((size_t)(v4 ? S / 4 : S), TALLY_MAX_BLOCKS);
  const dim3 g(nb), b(TALLY_THREADS);
  const hipStream_t st = as_stream(stream);
  switch (C) {
    case 1: launch_tallies<1>(mode, v4, g, b, st, p); break;
    case 2: launch_tallies<2>(mode, v4, g, b, st, p); break;
    case 3: launch_tallies<3>(mode, v4, g, b, st, p); break;
    case 4: launch_tallies<4>(mode, v4, g, b, st, p); break;
    case 5: launch_tallies<5>(mode, v4, g, b, st, p); break;
    case 6: launch_tallies<6>(mode, v4, g, b, st, p); break;
    case 7: launch_tallies<7>(mode, v4, g, b, st, p); break;
    default: launch_tallies<8>(mode, v4, g, b, st, p); break;
  }
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_seg_tallies_final, dim3(1), dim3(64), 0, as_stream(stream), p.partial, (int)nb, C, S, counts);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

size_t effq_label_tallies_ws_bytes(void) { return (size_t)LTALLY_MAX_BLOCKS * TALLY_NCNT * sizeof(uint32_t); }

int effq_label_tallies(const uint8_t* pred, const uint8_t* truth, int truth_planes, int C, long long S,
                       const uint16_t* lut, long long* counts, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(pred && truth && lut && counts && ws && C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(S > 0 && S < (1ll << 40));            // a workgroup's partial counts are 32-bit
  EFFQ_CHECK_WS(ws_bytes, effq_label_tallies_ws_bytes());
  LabelLut l;
  for (int v = 0; v < 256; ++v) l.v[v] = (uint16_t)(lut[v] & ((1u << C) - 1u));
  LabelTallyParams p;
  p.pred = pred; p.truth = truth; p.partial = static_cast<uint32_t*>(ws); p.S = S;
  const bool planes = truth_planes != 0;
  const bool v4 = ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(truth)) & 3) == 0 &&
                  (!planes || S % 4 == 0);
  const unsigned nb = grid_for((size_t)(v4 ? (S + 3) / 4 : S), LTALLY_MAX_BLOCKS);
  const dim3 g(nb);
  const hipStream_t st = as_stream(stream);
  switch (C) {
    case 1: launch_label_tallies<1>(planes, v4, g, st, p, l); break;
    case 2: launch_label_tallies<2>(planes, v4, g, st, p, l); break;
    case 3: launch_label_tallies<3>(planes, v4, g, st, p, l); break;
    case 4: launch_label_tallies<4>(planes, v4, g, st, p, l); break;
    case 5: launch_label_tallies<5>(planes, v4, g, st, p, l); break;
    case 6: launch_label_tallies<6>(planes, v4, g, st, p, l); break;
    case 7: launch_label_tallies<7>(planes, v4, g, st, p, l); break;
    default: launch_label_tallies<8>(planes, v4, g, st, p, l); break;
  }
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_seg_tallies_final, dim3(1), dim3(64), 0, st, p.partial, (int)nb, C, S, counts);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_seg_labels(const float* logits, int N, int C, long long S, int rule, int fuse, float thresh, int out_bytes,
                    void* out, void* stream) {
  EFFQ_CHECK_ARG(logits && out && N > 0 && N <= 65535 && S > 0 && C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(rule == EFFQ_SEG_LABEL_ARGMAX || rule == EFFQ_SEG_LABEL_BRATS || rule == EFFQ_SEG_LABEL_RANK ||
                 rule == EFFQ_SEG_LABEL_PLANES);
  EFFQ_CHECK_ARG(fuse == EFFQ_SEG_FUSE_NONE || fuse == EFFQ_SEG_FUSE_AGG || fuse == EFFQ_SEG_FUSE_CON);
  EFFQ_CHECK_ARG(rule != EFFQ_SEG_LABEL_ARGMAX || fuse == EFFQ_SEG_FUSE_NONE);
  EFFQ_CHECK_ARG(rule != EFFQ_SEG_LABEL_BRATS || C >= 3);
  EFFQ_CHECK_ARG(out_bytes == 1 || (out_bytes == 2 && rule != EFFQ_SEG_LABEL_PLANES));
  LabelParams p;
  p.logits = logits; p.out = out; p.S = S; p.fuse = fuse; p.thresh = thresh;
  const bool v4 = S % 4 == 0 && ((reinterpret_cast<uintptr_t>(logits) & 15) |
                                 (reinterpret_cast<uintptr_t>(out) & (4 * out_bytes - 1))) == 0;
  const dim3 g(grid_for((size_t)(v4 ? S / 4 : S), LABEL_MAX_BLOCKS), N);
  const hipStream_t st = as_stream(stream);
  const bool u16 = out_bytes == 2;
  switch (C) {
    case 1: launch_labels<1>(rule, u16, v4, g, st, p); break;
    case 2: launch_labels<2>(rule, u16, v4, g, st, p); break;
    case 3: launch_labels<3>(rule, u16, v4, g, st, p); break;
    case 4: launch_labels<4>(rule, u16, v4, g, st, p); break;
    case 5: launch_labels<5>(rule, u16, v4, g, st, p); break;
    case 6: launch_labels<6>(rule, u16, v4, g, st, p); break;
    case 7: launch_labels<7>(rule, u16, v4, g, st, p); break;
    default: launch_labels<8>(rule, u16, v4, g, st, p); break;
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
