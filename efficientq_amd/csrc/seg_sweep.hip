// Threshold sweep of the validation (evaluate.validate_seg(..., sweep=True), --thr_sweep): one pass over the stitched
// logits (C, S) of one case and its label that counts, for 4096 score bins at once, the labelled and the unlabelled voxels
// of every class: hist (C, 2, 4096) int64, hist[c][g][b] = the voxels with truth g for class c whose score for class c
// falls in bin b.  The suffix sums of a class over the bins k .. 4095 are the confusion counts of the decision "score >=
// edge k", so ROC, AUC and the best-Dice threshold follow on the host from integers (evaluate.sweep_summary).
//
// Scores (fp32, nothing fused):
//   sigmoid, fuse NONE  s_c = x_c
//   sigmoid, AGG        s_c = the largest non-NaN of x_c .. x_{C-1}, NaN when all are NaN
//   sigmoid, CON        s_c = the least of x_0 .. x_c, NaN when any is NaN
//   argmax              s_c = x_c - max_{j != c} x_j (one subtraction); the max is torch.max's, where NaN counts as the
//                       largest value, so a NaN in any other channel makes s_c NaN; C = 1: s_0 = x_0
// Edges: e_0 = -inf, e_k = (k - 2048) / 128 for k = 1 .. 4095 (exact in fp32), except e_2048 = `thresh` in sigmoid mode
// (the decision threshold of the tallies, about -1.78e-7) and 0 in argmax mode.  bin(s) = the number of k >= 1 with
// e_k <= s; NaN -> 0.  With that edge bin >= 2048 is bit c of predict<SIGMOID, C> (seg_decide.h).  In argmax mode the bin
// is then pinned to the decision of predict<ARGMAX, C>: max(bin, 2048) for the class it names, min(bin, 2047) for every
// other; that moves only margin-0 ties and voxels with a NaN, to where torch.max puts them.
// The bin is found from clamp((s + 16) * 128), whose fp32 add can round across an edge, followed by one step down and
// one step up against the exact edges (sweep_edge): the edges are the definition.
//
// Kernel: a workgroup of 512 threads owns a range of voxels (gridDim.x, capped: it loops) and two classes (gridDim.y =
// ceil(C / 2)): 2 classes x 2 truths x 4096 bins of 32-bit counters = 64 KB of LDS, private to the workgroup (it sees fewer
// than 2^31 voxels).  Sigmoid mode without fuse reads only its own two channels; with a fuse and in argmax mode a score
// needs the other channels too, so the C channels are read once per class pair.  16-B loads for the voxels 0 .. 4 (S / 4)
// - 1 through a type of 4-B alignment (the planes of an odd S do not start on 16 B); the last S % 4 voxels are taken one
// by one by the first wave of workgroup 0.  Most lanes of a wave hit the same few bins (background), so before the LDS
// atomic equal keys of a wave are combined by ballot, as k_cc_accum does: up to four distinct keys, whose leaders add their
// lane counts, and one add per lane beyond.  At the end every workgroup adds its non-zero counters to hist with 64-bit
// integer atomics; hist is zeroed by a first launch.  Integer adds only: equal inputs give equal bits whatever the
// schedule.  Two launches on `stream`, no read by the host, no workgroup that waits for another.
#include <math.h>
#include "common.h"
#include "seg_decide.h"

namespace effq {

constexpr int SWEEP_BINS = EFFQ_SEG_SWEEP_BINS;
constexpr int SWEEP_MID = SWEEP_BINS / 2;                 // the bin of the decision: edge 2048
constexpr int SWEEP_THREADS = 512;
constexpr int SWEEP_MAX_BLOCKS = 256;                     // voxel ranges; x class pairs: two workgroups of 64 KB per CU
constexpr int SWEEP_MATCH_ROUNDS = 4;                     // distinct keys of a wave that are combined by ballot
constexpr int SWEEP_SLOTS = 2 * 2 * SWEEP_BINS;           // LDS counters: (class of the pair, truth, bin)
static_assert(SWEEP_BINS == 4096 && SWEEP_SLOTS * sizeof(uint32_t) == 65536, "64 KB of static LDS");
static_assert(SWEEP_SLOTS % SWEEP_THREADS == 0 && SWEEP_THREADS % 64 == 0, "whole waves, whole flush trips");

struct SweepParams {
  const float* logits;    // (C, S)
  const uint8_t* label;   // (S) class ids for argmax, (C, S) 0/1 for multi-label
  long long* hist;        // (C, 2, 4096)
  long long S;
  int fuse;
  float thresh;           // edge 2048: the decision threshold in sigmoid mode, 0 in argmax mode
};

struct __attribute__((packed, aligned(4))) SweepFloat4 { float x, y, z, w; };    // 16 B at any 4-B boundary
struct __attribute__((packed, aligned(1))) SweepByte4 { uint8_t x, y, z, w; };

// edge k for k = 1 .. 4095
__host__ __device__ __forceinline__ float sweep_edge(int k, float mid) {
  return k == SWEEP_MID ? mid : (float)(k - SWEEP_MID) * 0.0078125f;
}

// the number of k in 1 .. 4095 with edge k <= s; NaN -> 0
__device__ __forceinline__ int sweep_bin(float s, float mid) {
  float t = (s + 16.0f) * 128.0f;
  t = fminf(fmaxf(t, 0.0f), (float)(SWEEP_BINS - 1));     // fmaxf(NaN, 0) = 0
  int k = (int)t;
  if (k >= 1 && !(sweep_edge(k, mid) <= s)) --k;
  if (k < SWEEP_BINS - 1 && sweep_edge(k + 1, mid) <= s) ++k;
  return k;
}

// torch.max's order on two values: NaN is the largest
__device__ __forceinline__ float sweep_max_nan(float a, float b) {
  return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b);
}
__device__ __forceinline__ float sweep_min_nan(float a, float b) {
  return (a != a || b != b) ? __builtin_nanf("") : fminf(a, b);
}

// the score of class c (c uniform in the workgroup, the loops static: no indexed register array) from the C logits of a
// voxel, in argmax mode or with a fuse
template <int MODE, int C>
__device__ __forceinline__ float sweep_score(const float* v, int c, int fuse) {
  float x = v[0];
#pragma unroll
  for (int j = 1; j < C; ++j) x = j == c ? v[j] : x;
  if constexpr (MODE == EFFQ_SEG_ARGMAX) {
    if constexpr (C == 1) return x;
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < C; ++j) m = j == c ? m : sweep_max_nan(m, v[j]);
    return x - m;
  } else {
    if (fuse == EFFQ_SEG_FUSE_AGG) {
      float m = __builtin_nanf("");                        // fmaxf keeps the value that is not NaN
#pragma unroll
      for (int j = 0; j < C; ++j) m = j >= c ? fmaxf(m, v[j]) : m;
      return m;
    }
    if (fuse == EFFQ_SEG_FUSE_CON) {
      float m = INFINITY;
#pragma unroll
      for (int j = 0; j < C; ++j) m = j <= c ? sweep_min_nan(m, v[j]) : m;
      return m;
    }
    return x;
  }
}

// adds one key per valid lane to the LDS counters; every lane of the wave calls it (the ballots need them all).
// This is wave_match_count (common.h) written out: through the helper k_seg_sweep gets another register allocation, and
// two of six timed cases were slower than the previous build by more than its spread (profiles/seg_cc_split_ab.txt).
__device__ __forceinline__ void sweep_add(uint32_t* s_hist, bool valid, uint32_t key, int lane) {
  unsigned long long todo = __ballot(valid);
  uint32_t add = 0;                                       // the leader of a group carries the group's count
  for (int round = 0; round < SWEEP_MATCH_ROUNDS && todo; ++round) {
    const int lead = __ffsll((long long)todo) - 1;
    const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, lead);
    const unsigned long long m = __ballot(key == k) & todo;
    if (lane == lead) add = (uint32_t)__popcll(m);
    todo &= ~m;
  }
  if ((todo >> lane) & 1ull) add = 1;                     // more distinct keys than rounds: one add per voxel
  if (add) atomicAdd(&s_hist[key], add);
}

// one voxel of the pair's classes ca (slot 0) and, when `two`, ca + 1 (slot 1): scores sa / sb, truth bits ga / gb,
// pred: the decision of predict<ARGMAX, C> (argmax mode only)
template <int MODE>
__device__ __forceinline__ void sweep_voxel(uint32_t* s_hist, bool valid, bool two, int ca, float sa, float sb,
                                            uint32_t ga, uint32_t gb, uint32_t pred, float mid, int lane) {
  int ba = sweep_bin(sa, mid), bb = sweep_bin(sb, mid);
  if constexpr (MODE == EFFQ_SEG_ARGMAX) {
    ba = (pred >> ca) & 1u ? max(ba, SWEEP_MID) : min(ba, SWEEP_MID - 1);
    bb = (pred >> (ca + 1)) & 1u ? max(bb, SWEEP_MID) : min(bb, SWEEP_MID - 1);
  }
  sweep_add(s_hist, valid, ga * SWEEP_BINS + (uint32_t)ba, lane);
  if (two) sweep_add(s_hist, valid, (2u + gb) * SWEEP_BINS + (uint32_t)bb, lane);
}

template <int MODE, int C>
__global__ __launch_bounds__(SWEEP_THREADS) void k_seg_sweep(SweepParams p) {
  __shared__ uint32_t s_hist[SWEEP_SLOTS];
  for (int k = threadIdx.x; k < SWEEP_SLOTS; k += SWEEP_THREADS) s_hist[k] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int ca = 2 * blockIdx.y, cb = ca + 1 < C ? ca + 1 : ca;    // cb == ca: the pair holds one class
  const bool two = ca + 1 < C;
  const bool all = MODE == EFFQ_SEG_ARGMAX || p.fuse != EFFQ_SEG_FUSE_NONE;     // a score needs the other channels
  const long long groups = p.S / 4;
  // the trip count is the same for every lane of the workgroup: the ballots need whole waves
  for (long long g0 = (long long)blockIdx.x * SWEEP_THREADS; g0 < groups; g0 += (long long)gridDim.x * SWEEP_THREADS) {
    const long long g = g0 + threadIdx.x;
    const bool valid = g < groups;
    float sa[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t ga[4] = {0, 0, 0, 0}, gb[4] = {0, 0, 0, 0}, pred[4] = {0, 0, 0, 0};
    if (valid) {
      if (all) {
        float v[4][C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const SweepFloat4 f = *reinterpret_cast<const SweepFloat4*>(p.logits + c * p.S + g * 4);
          v[0][c] = f.x; v[1][c] = f.y; v[2][c] = f.z; v[3][c] = f.w;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          sa[u] = sweep_score<MODE, C>(v[u], ca, p.fuse);
          sb[u] = sweep_score<MODE, C>(v[u], cb, p.fuse);
          if constexpr (MODE == EFFQ_SEG_ARGMAX) pred[u] = predict<MODE, C>(v[u], p.fuse, p.thresh);
        }
      } else {
        const SweepFloat4 fa = *reinterpret_cast<const SweepFloat4*>(p.logits + ca * p.S + g * 4);
        const SweepFloat4 fb = *reinterpret_cast<const SweepFloat4*>(p.logits + cb * p.S + g * 4);
        sa[0] = fa.x; sa[1] = fa.y; sa[2] = fa.z; sa[3] = fa.w;
        sb[0] = fb.x; sb[1] = fb.y; sb[2] = fb.z; sb[3] = fb.w;
      }
      if constexpr (MODE == EFFQ_SEG_ARGMAX) {
        const SweepByte4 l = *reinterpret_cast<const SweepByte4*>(p.label + g * 4);
        const int lab[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          ga[u] = lab[u] == ca ? 1u : 0u;
          gb[u] = lab[u] == cb ? 1u : 0u;
        }
      } else {
        const SweepByte4 la = *reinterpret_cast<const SweepByte4*>(p.label + ca * p.S + g * 4);
        const SweepByte4 lb = *reinterpret_cast<const SweepByte4*>(p.label + cb * p.S + g * 4);
        ga[0] = la.x != 0; ga[1] = la.y != 0; ga[2] = la.z != 0; ga[3] = la.w != 0;
        gb[0] = lb.x != 0; gb[1] = lb.y != 0; gb[2] = lb.z != 0; gb[3] = lb.w != 0;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      sweep_voxel<MODE>(s_hist, valid, two, ca, sa[u], sb[u], ga[u], gb[u], pred[u], p.thresh, lane);
  }
  // the last S % 4 voxels, one each for the first lanes of the first wave of workgroup 0
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const long long t = groups * 4 + lane;
    const bool valid = t < p.S;
    float sa = 0.f, sb = 0.f;
    uint32_t ga = 0, gb = 0, pred = 0;
    if (valid) {
      if (all) {
        float v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = p.logits[c * p.S + t];
        sa = sweep_score<MODE, C>(v, ca, p.fuse);
        sb = sweep_score<MODE, C>(v, cb, p.fuse);
        if constexpr (MODE == EFFQ_SEG_ARGMAX) pred = predict<MODE, C>(v, p.fuse, p.thresh);
      } else {
        sa = p.logits[ca * p.S + t];
        sb = p.logits[cb * p.S + t];
      }
      if constexpr (MODE == EFFQ_SEG_ARGMAX) {
        const int lab = p.label[t];
        ga = lab == ca ? 1u : 0u;
        gb = lab == cb ? 1u : 0u;
      } else {
        ga = p.label[ca * p.S + t] != 0;
        gb = p.label[cb * p.S + t] != 0;
      }
    }
    sweep_voxel<MODE>(s_hist, valid, two, ca, sa, sb, ga, gb, pred, p.thresh, lane);
  }
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(p.hist) + (size_t)ca * 2 * SWEEP_BINS;
  const int slots = two ? SWEEP_SLOTS : SWEEP_SLOTS / 2;
  for (int k = threadIdx.x; k < slots; k += SWEEP_THREADS) {
    const uint32_t n = s_hist[k];
    if (n) atomicAdd(&out[k], (unsigned long long)n);
  }
}

__global__ __launch_bounds__(256) void k_seg_sweep_zero(long long* __restrict__ hist, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) hist[i] = 0;
}

template <int C>
static void launch_sweep(int mode, dim3 g, hipStream_t st, const SweepParams& p) {
  if (mode == EFFQ_SEG_ARGMAX)
    hipLaunchKernelGGL((k_seg_sweep<EFFQ_SEG_ARGMAX, C>), g, dim3(SWEEP_THREADS), 0, st, p);
  else
    hipLaunchKernelGGL((k_seg_sweep<EFFQ_SEG_SIGMOID, C>), g, dim3(SWEEP_THREADS), 0, st, p);
}

// the voxel ranges (gridDim.x) of a case of S voxels and the trips of a workgroup over its groups of four voxels
static void sweep_plan(long long S, int* nb, int* trips) {
  const long long groups = S / 4;
  long long b = (groups + SWEEP_THREADS - 1) / SWEEP_THREADS;
  b = b < 1 ? 1 : (b > SWEEP_MAX_BLOCKS ? SWEEP_MAX_BLOCKS : b);
  *nb = (int)b;
  *trips = (int)((groups + b * SWEEP_THREADS - 1) / (b * SWEEP_THREADS));
}

static bool sweep_mid_ok(int mode, float thresh) {
  // strictly between edge 2047 and edge 2049 (NaN fails both comparisons); argmax mode has no threshold: its edge is 0
  return mode == EFFQ_SEG_ARGMAX || (thresh > -0.0078125f && thresh < 0.0078125f);
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_seg_sweep_edges(int mode, float thresh, float* edges_host) {
  EFFQ_CHECK_ARG(edges_host && (mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID));
  EFFQ_CHECK_ARG(sweep_mid_ok(mode, thresh));
  const float mid = mode == EFFQ_SEG_ARGMAX ? 0.0f : thresh;
  edges_host[0] = -INFINITY;
  for (int k = 1; k < SWEEP_BINS; ++k) edges_host[k] = sweep_edge(k, mid);
  return EFFQ_OK;
}

int effq_seg_sweep_plan(int C, long long S, int mode, int* grid, int* trips) {
  EFFQ_CHECK_ARG(grid && trips && C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES && S > 0 && S < (1ll << 31));
  EFFQ_CHECK_ARG(mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID);
  int nb = 0;
  sweep_plan(S, &nb, trips);
  *grid = nb * ((C + 1) / 2);
  return EFFQ_OK;
}

int effq_seg_sweep(const float* logits, const uint8_t* label, int C, long long S, int mode, int fuse, float thresh,
                   long long* hist, void* stream) {
  EFFQ_CHECK_ARG(logits && label && hist && C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES && S > 0 && S < (1ll << 31));
  EFFQ_CHECK_ARG(mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID);
  EFFQ_CHECK_ARG(fuse == EFFQ_SEG_FUSE_NONE || fuse == EFFQ_SEG_FUSE_AGG || fuse == EFFQ_SEG_FUSE_CON);
  EFFQ_CHECK_ARG(mode != EFFQ_SEG_ARGMAX || fuse == EFFQ_SEG_FUSE_NONE);
  EFFQ_CHECK_ARG(sweep_mid_ok(mode, thresh));
  EFFQ_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 3) == 0 && (reinterpret_cast<uintptr_t>(hist) & 7) == 0);
  SweepParams p;
  p.logits = logits; p.label = label; p.hist = hist; p.S = S; p.fuse = fuse;
  p.thresh = mode == EFFQ_SEG_ARGMAX ? 0.0f : thresh;
  int nb = 0, trips = 0;
  sweep_plan(S, &nb, &trips);
  const hipStream_t st = as_stream(stream);
  const int n = C * 2 * SWEEP_BINS;
  hipLaunchKernelGGL(k_seg_sweep_zero, dim3((n + 255) / 256), dim3(256), 0, st, hist, n);
  EFFQ_LAUNCH_CHECK();
  const dim3 g(nb, (C + 1) / 2);
  switch (C) {
    case 1: launch_sweep<1>(mode, g, st, p); break;
    case 2: launch_sweep<2>(mode, g, st, p); break;
    case 3: launch_sweep<3>(mode, g, st, p); break;
    case 4: launch_sweep<4>(mode, g, st, p); break;
    case 5: launch_sweep<5>(mode, g, st, p); break;
    case 6: launch_sweep<6>(mode, g, st, p); break;
    case 7: launch_sweep<7>(mode, g, st, p); break;
    default: launch_sweep<8>(mode, g, st, p); break;
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
