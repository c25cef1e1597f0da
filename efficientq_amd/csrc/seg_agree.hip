// Agreement of two networks on one case (evaluate.validate_seg(..., fp_model=...), --vs_fp): the stitched last-head logits
// of the calibrated and of the full-precision network, (C, S) fp32 each, are read once, and every voxel of both is decided
// by predict<MODE, C> (seg_decide.h) - the rule of the tallies, the label maps and the lesion counts.  Out come the
// confusion counts with the FP network's decision as the truth, the voxels decided differently in any class, per class
// sum (q - f)^2, sum f^2, max |q - f| and sum |p_q - p_f| in fp64 (p = the sigmoid of the channel, or the softmax over the
// channels in argmax mode), and optionally one byte per voxel with bit c set where class c is decided differently.
//
// Two launches: per-workgroup partials, then one workgroup adds them in block order (the scheme of k_seg_tallies).  The
// grid depends on S alone, every thread adds its voxels in index order, the wave and block trees are fixed and there is no
// floating-point atomic: equal inputs give equal bits.  16-B loads per channel for the voxels 0 .. 4 (S / 4) - 1, through
// a type of 4-B alignment, since with S % 4 != 0 the channel planes do not start on 16 B; the last S % 4 voxels are read
// one by one.  2 C S floats are read; the fp64 exponentials (2 C per voxel) are the arithmetic.
#include "common.h"
#include "seg_decide.h"

namespace effq {

constexpr int AGREE_THREADS = 256;
constexpr int AGREE_WAVES = AGREE_THREADS / 64;
constexpr int AGREE_MAX_BLOCKS = 768;     // 3 workgroups per CU: 3 waves per SIMD to hide the fp64 chains
constexpr int AGREE_MAXC = EFFQ_SEG_TALLIES_MAX_CLASSES;
constexpr int AGREE_NSTAT = 4 * AGREE_MAXC;       // per class: sum (q - f)^2, sum f^2, max |q - f|, sum |p_q - p_f|
constexpr int AGREE_NCNT = 3 * AGREE_MAXC + 1;    // per class: both, Q positive, FP positive; then the flipped voxels
static_assert((size_t)AGREE_MAX_BLOCKS * (AGREE_NSTAT * sizeof(double) + AGREE_NCNT * sizeof(uint32_t)) <=
                  EFFQ_SEG_AGREEMENT_WS_BYTES, "workspace");

struct AgreeParams {
  const float* q;       // (C, S) logits of the calibrated network
  const float* f;       // (C, S) logits of the FP network
  uint8_t* map;         // (S) or null
  double* pstat;        // (gridDim.x, 4 C)
  uint32_t* pcnt;       // (gridDim.x, 3 C + 1)
  long long S;
  int fuse;
  float thresh;
};

struct __attribute__((packed, aligned(4))) Float4U { float x, y, z, w; };    // 16 B at any 4-B boundary
struct __attribute__((packed, aligned(1))) Byte4U { uint8_t x, y, z, w; };

// per-thread running values of one workgroup's share
template <int C>
struct AgreeAcc {
  double st[4 * C];
  uint32_t cnt[3 * C + 1];
};

// one voxel of both networks: decisions, counts and the fp64 sums; returns the classes decided differently
template <int MODE, int C>
__device__ __forceinline__ uint32_t agree_voxel(const float* q, const float* f, int fuse, float thresh, AgreeAcc<C>& a) {
  const uint32_t pq = predict<MODE, C>(q, fuse, thresh), pf = predict<MODE, C>(f, fuse, thresh);
  const uint32_t x = pq ^ pf;
  a.cnt[3 * C] += x != 0 ? 1u : 0u;
  double eq[C], ef[C], sq = 0.0, sf = 0.0;
  if constexpr (MODE == EFFQ_SEG_ARGMAX) {          // softmax over the channels: exp(x - max) / sum
    float mq = q[0], mf = f[0];
#pragma unroll
    for (int c = 1; c < C; ++c) {
      mq = fmaxf(mq, q[c]);
      mf = fmaxf(mf, f[c]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      eq[c] = exp((double)q[c] - (double)mq);
      ef[c] = exp((double)f[c] - (double)mf);
      sq += eq[c];
      sf += ef[c];
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    a.cnt[3 * c + 0] += (pq >> c) & (pf >> c) & 1u;
    a.cnt[3 * c + 1] += (pq >> c) & 1u;
    a.cnt[3 * c + 2] += (pf >> c) & 1u;
    const double dq = (double)q[c], df = (double)f[c], d = dq - df;
    a.st[4 * c + 0] += d * d;
    a.st[4 * c + 1] += df * df;
    a.st[4 * c + 2] = fmax(a.st[4 * c + 2], fabs(d));
    double dp;
    if constexpr (MODE == EFFQ_SEG_ARGMAX)
      dp = eq[c] / sq - ef[c] / sf;
    else                                            // the channel's sigmoid, before any merge
      dp = 1.0 / (1.0 + exp(-dq)) - 1.0 / (1.0 + exp(-df));
    a.st[4 * c + 3] += fabs(dp);
  }
  return x;
}

template <int MODE, int C>
__global__ __launch_bounds__(AGREE_THREADS) void k_seg_agreement(AgreeParams p) {
  AgreeAcc<C> a;
#pragma unroll
  for (int k = 0; k < 4 * C; ++k) a.st[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 3 * C + 1; ++k) a.cnt[k] = 0;
  const long long groups = p.S / 4;
  for (long long g = (long long)blockIdx.x * AGREE_THREADS + threadIdx.x; g < groups;
       g += (long long)gridDim.x * AGREE_THREADS) {
    float q[4][C], f[4][C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const Float4U a4 = *reinterpret_cast<const Float4U*>(p.q + c * p.S + g * 4);
      const Float4U b4 = *reinterpret_cast<const Float4U*>(p.f + c * p.S + g * 4);
      q[0][c] = a4.x; q[1][c] = a4.y; q[2][c] = a4.z; q[3][c] = a4.w;
      f[0][c] = b4.x; f[1][c] = b4.y; f[2][c] = b4.z; f[3][c] = b4.w;
    }
    uint32_t x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = agree_voxel<MODE, C>(q[u], f[u], p.fuse, p.thresh, a);
    if (p.map) {
      Byte4U b;
      b.x = (uint8_t)x[0]; b.y = (uint8_t)x[1]; b.z = (uint8_t)x[2]; b.w = (uint8_t)x[3];
      *reinterpret_cast<Byte4U*>(p.map + g * 4) = b;
    }
  }
  // the last S % 4 voxels, one each for the first threads of workgroup 0, after their own groups
  const long long t = groups * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < p.S) {
    float q[C], f[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      q[c] = p.q[c * p.S + t];
      f[c] = p.f[c * p.S + t];
    }
    const uint32_t x = agree_voxel<MODE, C>(q, f, p.fuse, p.thresh, a);
    if (p.map) p.map[t] = (uint8_t)x;
  }
  __shared__ double rs[AGREE_WAVES][4 * C];
  __shared__ uint32_t rc[AGREE_WAVES][3 * C + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4 * C; ++k) {
    double v = a.st[k];
    if ((k & 3) == 2) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));      // the tree of wave_sum_all
    } else {
      v = wave_sum_all(v);
    }
    if (lane == 0) rs[wave][k] = v;
  }
#pragma unroll
  for (int k = 0; k < 3 * C + 1; ++k) {
    const uint32_t s = wave_sum_all(a.cnt[k]);
    if (lane == 0) rc[wave][k] = s;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < 4 * C) {
    double v = rs[0][k];
    for (int w = 1; w < AGREE_WAVES; ++w) v = (k & 3) == 2 ? fmax(v, rs[w][k]) : v + rs[w][k];
    p.pstat[(size_t)blockIdx.x * 4 * C + k] = v;
  }
  if (k < 3 * C + 1) {
    uint32_t s = 0;
    for (int w = 0; w < AGREE_WAVES; ++w) s += rc[w][k];
    p.pcnt[(size_t)blockIdx.x * (3 * C + 1) + k] = s;
  }
}

// threads 0 .. 4 C - 1 fold the fp64 partials, threads 64 .. 64 + 3 C the counts, both in block order;
// counts (C, 4) = both, Q only, FP only, neither
__global__ __launch_bounds__(128) void k_seg_agreement_final(const double* __restrict__ pstat,
                                                             const uint32_t* __restrict__ pcnt, int nblocks, int C,
                                                             long long S, long long* __restrict__ counts,
                                                             long long* __restrict__ flips, double* __restrict__ stats) {
  __shared__ long long tot[AGREE_NCNT];
  const int k = threadIdx.x;
  if (k < 4 * C) {
    double v = pstat[k];
    for (int b = 1; b < nblocks; ++b) {
      const double w = pstat[(size_t)b * 4 * C + k];
      v = (k & 3) == 2 ? fmax(v, w) : v + w;
    }
    stats[k] = v;
  }
  const int j = k - 64;
  if (j >= 0 && j < 3 * C + 1) {
    long long s = 0;
    for (int b = 0; b < nblocks; ++b) s += pcnt[(size_t)b * (3 * C + 1) + j];
    tot[j] = s;
  }
  __syncthreads();
  if (k < C) {
    const long long both = tot[3 * k], qp = tot[3 * k + 1], fp = tot[3 * k + 2];
    counts[4 * k + 0] = both;
    counts[4 * k + 1] = qp - both;
    counts[4 * k + 2] = fp - both;
    counts[4 * k + 3] = S - qp - fp + both;
  }
  if (k == 0) flips[0] = tot[3 * C];
}

template <int C>
static void launch_agreement(int mode, dim3 g, hipStream_t st, const AgreeParams& p) {
  if (mode == EFFQ_SEG_ARGMAX)
    hipLaunchKernelGGL((k_seg_agreement<EFFQ_SEG_ARGMAX, C>), g, dim3(AGREE_THREADS), 0, st, p);
  else
    hipLaunchKernelGGL((k_seg_agreement<EFFQ_SEG_SIGMOID, C>), g, dim3(AGREE_THREADS), 0, st, p);
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_seg_agreement(const float* logits_q, const float* logits_fp, int C, long long S, int mode, int fuse,
                       float thresh, long long* counts, long long* flips, double* stats, uint8_t* map, void* ws,
                       size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(logits_q && logits_fp && counts && flips && stats && ws && S > 0 && C > 0 &&
                 C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID);
  EFFQ_CHECK_ARG(fuse == EFFQ_SEG_FUSE_NONE || fuse == EFFQ_SEG_FUSE_AGG || fuse == EFFQ_SEG_FUSE_CON);
  EFFQ_CHECK_ARG(ws_bytes >= EFFQ_SEG_AGREEMENT_WS_BYTES);
  EFFQ_CHECK_ARG(((reinterpret_cast<uintptr_t>(logits_q) | reinterpret_cast<uintptr_t>(logits_fp)) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(ws) & 7) == 0);
  size_t nb = ((size_t)(S / 4) + AGREE_THREADS - 1) / AGREE_THREADS;
  nb = nb < 1 ? 1 : (nb > (size_t)AGREE_MAX_BLOCKS ? (size_t)AGREE_MAX_BLOCKS : nb);
  AgreeParams p;
  p.q = logits_q; p.f = logits_fp; p.map = map; p.S = S; p.fuse = fuse; p.thresh = thresh;
  p.pstat = static_cast<double*>(ws);
  p.pcnt = reinterpret_cast<uint32_t*>(p.pstat + (size_t)AGREE_MAX_BLOCKS * AGREE_NSTAT);
  const dim3 g((unsigned)nb);
  const hipStream_t st = as_stream(stream);
  switch (C) {
    case 1: launch_agreement<1>(mode, g, st, p); break;
    case 2: launch_agreement<2>(mode, g, st, p); break;
    case 3: launch_agreement<3>(mode, g, st, p); break;
    case 4: launch_agreement<4>(mode, g, st, p); break;
    case 5: launch_agreement<5>(mode, g, st, p); break;
    case 6: launch_agreement<6>(mode, g, st, p); break;
    case 7: launch_agreement<7>(mode, g, st, p); break;
    default: launch_agreement<8>(mode, g, st, p); break;
  }
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_seg_agreement_final, dim3(1), dim3(128), 0, st, p.pstat, p.pcnt, (int)nb, C, S, counts, flips,
                     stats);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
