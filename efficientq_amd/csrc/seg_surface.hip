// The exact Euclidean distance transform of 3-D masks and the surface-distance columns of the validation
// (validate_seg(..., surface=True): hd, hd95, assd per class, in voxel units).  The transform is separable and all of
// it is integer arithmetic, so the squared distance map is exact by construction.  Phases of a call:
//
//   masks    (effq_seg_surface only) decide<MODE, C> of every voxel -> 16 decision bits per voxel (seg_masks.h)
//   surface  (effq_seg_surface only, seg_surf.h) a 6-neighbour stencil on the bits of all 2 C masks at once: a voxel of a mask is a
//            surface voxel when a face neighbour is background or lies outside the volume
//   rows, lines   the three separable passes of seg_surf.h with the metric EdtVox: squared distances in int32
//   reduce   (effq_seg_surface only) every surface voxel of one mask reads the other mask's map: integer atomicAdd on a
//            histogram over squared distance per class and direction (the crowded bins first in LDS), then one
//            workgroup per class walks its two histograms in ascending order for the counts, the maxima, the fp64 sums
//            of square roots and the two pooled order statistics
//
// Integer adds commute, and the walk adds its fp64 terms in a fixed order: equal inputs give equal bits.  A fixed number
// of launches on `stream`, no read by the host, no workgroup that waits for another.
#include "common.h"
#include "seg_decide.h"
#include "seg_masks.h"
#include "seg_surf.h"

namespace effq {

constexpr int EDT_LDS_MAX = 64 * 1024;                 // the slab is narrowed down to EDT_LDS_AIM (seg_surf.h); a single line may take this
constexpr int SURF_LOW = 256;                          // squared distances below this are counted in LDS first
constexpr int SURF_FINAL_THREADS = 1024;
static_assert(EFFQ_EDT_MAX_LINE == EDT_LDS_MAX / 4 - 2, "one line and its range fit the LDS of a workgroup");

static inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

static inline long long edt_max_sq(int D, int H, int W) {
  return (long long)(D - 1) * (D - 1) + (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1);
}

struct SurfWs {
  int* sq;             // (P, S)
  uint16_t* bits;      // (S)
  uint16_t* surf;      // (S)
  uint32_t* hist;      // (P, nbins + 1): the last bin counts the voxels whose target mask has no surface
  size_t hist_bytes;
  size_t bytes;
};

static SurfWs surf_ws(void* ws, int P, int D, int H, int W) {
  SurfWs r;
  const size_t S = (size_t)D * H * W;
  char* p = static_cast<char*>(ws);
  size_t off = 0;
  r.sq = reinterpret_cast<int*>(p + off);        off += align16((size_t)P * S * sizeof(int));
  r.bits = reinterpret_cast<uint16_t*>(p + off); off += align16(S * sizeof(uint16_t));
  r.surf = reinterpret_cast<uint16_t*>(p + off); off += align16(S * sizeof(uint16_t));
  r.hist_bytes = (size_t)P * (size_t)(edt_max_sq(D, H, W) + 2) * sizeof(uint32_t);
  r.hist = reinterpret_cast<uint32_t*>(p + off); off += align16(r.hist_bytes);
  r.bytes = off;
  return r;
}

// ---- reduce ---------------------------------------------------------------------------------------------------------
// hist (2 C, nbins + 1): row 2 c counts E_L over S(P) of class c, row 2 c + 1 counts E_P over S(L).  Dynamic LDS:
// 2 C * (SURF_LOW + 1) counters - the bins below SURF_LOW and the last bin (EDT_INF: the target has no surface), the
// ones that many voxels share
__global__ __launch_bounds__(CC_THREADS) void k_surf_hist(const uint16_t* __restrict__ surf, const int* __restrict__ sq,
                                                          int C, int S, long long nbins, uint32_t* __restrict__ hist) {
  extern __shared__ uint32_t s_low[];
  constexpr int SLOTS = SURF_LOW + 1;
  for (int k = threadIdx.x; k < 2 * C * SLOTS; k += CC_THREADS) s_low[k] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const uint32_t b = surf[i];
    if (!b) continue;
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int dir = 0; dir < 2; ++dir) {
        if (!((b >> (dir ? 8 + c : c)) & 1)) continue;
        const uint32_t e = (uint32_t)sq[(size_t)(dir ? c : C + c) * S + i];      // the other mask's map
        const int row = 2 * c + dir;
        if (e < (uint32_t)SURF_LOW) atomicAdd(&s_low[row * SLOTS + e], 1u);
        else if (e >= nbins) atomicAdd(&s_low[row * SLOTS + SURF_LOW], 1u);        // EDT_INF
        else atomicAdd(&hist[(size_t)row * (nbins + 1) + e], 1u);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * C * SLOTS; k += CC_THREADS) {
    const uint32_t n = s_low[k];
    const int slot = k % SLOTS;
    if (n) atomicAdd(&hist[(size_t)(k / SLOTS) * (nbins + 1) + (slot == SURF_LOW ? nbins : (long long)slot)], n);
  }
}

// One workgroup per class.  Thread t owns the bins [t * chunk, (t + 1) * chunk) of both histograms of its class: it
// counts them, keeps the largest occupied bin and adds count * sqrt(bin) in ascending order; thread 0 adds the threads'
// results in thread order and places the two pooled ranks; the threads that hold a rank walk their bins once more.
__global__ __launch_bounds__(SURF_FINAL_THREADS) void k_surf_final(const uint32_t* __restrict__ hist, long long nbins,
                                                                   long long* __restrict__ counts,
                                                                   double* __restrict__ sums) {
  constexpr int T = SURF_FINAL_THREADS;
  __shared__ unsigned long long s_n[2][T];
  __shared__ long long s_max[2][T];
  __shared__ double s_sum[2][T];
  __shared__ unsigned long long s_rank[2];
  __shared__ int s_pooled;
  const int c = blockIdx.x, t = threadIdx.x;
  const uint32_t* h[2] = {hist + (size_t)(2 * c) * (nbins + 1), hist + (size_t)(2 * c + 1) * (nbins + 1)};
  const long long chunk = (nbins + T - 1) / T;
  const long long b0 = min(nbins, t * chunk), b1 = min(nbins, b0 + chunk);
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    unsigned long long n = 0;
    long long mx = 0;
    double sum = 0.0;
    for (long long b = b0; b < b1; ++b) {
      const uint32_t k = h[dir][b];
      if (!k) continue;
      n += k;
      mx = b;
      sum += (double)k * sqrt((double)b);
    }
    s_n[dir][t] = n;
    s_max[dir][t] = mx;
    s_sum[dir][t] = sum;
  }
  __syncthreads();
  if (t == 0) {
    long long out[6] = {0, 0, 0, 0, 0, 0};
    for (int dir = 0; dir < 2; ++dir) {
      unsigned long long n = 0;
      long long mx = 0;
      double sum = 0.0;
      for (int k = 0; k < T; ++k) {
        n += s_n[dir][k];
        mx = max(mx, s_max[dir][k]);
        sum += s_sum[dir][k];
      }
      out[dir] = (long long)(n + h[dir][nbins]);
      out[2 + dir] = mx;
      sums[2 * c + dir] = sum;
    }
    const bool pooled = out[0] > 0 && out[1] > 0;      // then neither target is empty: every distance is in a bin
    if (pooled) {
      const unsigned long long n = (unsigned long long)(out[0] + out[1]);
      s_rank[0] = 95ull * (n - 1) / 100ull;
      s_rank[1] = min(s_rank[0] + 1, n - 1);
    }
    s_pooled = pooled;
    for (int k = 0; k < 4; ++k) counts[6 * c + k] = out[k];
    if (!pooled) counts[6 * c + 4] = counts[6 * c + 5] = 0;
    // s_n[0] becomes the number of pooled values in front of each thread's bins
    unsigned long long before = 0;
    for (int k = 0; k < T; ++k) {
      const unsigned long long mine = s_n[0][k] + s_n[1][k];
      s_n[0][k] = before;
      s_n[1][k] = mine;
      before += mine;
    }
  }
  __syncthreads();
  if (!s_pooled) return;
  unsigned long long seen = s_n[0][t];
  const unsigned long long end = seen + s_n[1][t];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const unsigned long long rank = s_rank[q];
    if (rank < seen || rank >= end) continue;
    unsigned long long at = seen;
    for (long long b = b0; b < b1; ++b) {
      at += (unsigned long long)h[0][b] + h[1][b];
      if (rank < at) {
        counts[6 * c + 4 + q] = b;
        break;
      }
    }
  }
}

}  // namespace effq
using namespace effq;

extern "C" {

size_t effq_surf_ws_bytes(int P, int D, int H, int W) {
  if (!edt_dims_ok(P, D, H, W)) return 0;
  return surf_ws(nullptr, P, D, H, W).bytes;
}

int effq_edt_sq(const uint8_t* masks, int P, int D, int H, int W, int32_t* sq, void* ws, size_t ws_bytes,
                void* stream) {
  EFFQ_CHECK_ARG(masks && sq && ws);
  EFFQ_CHECK_ARG(edt_dims_ok(P, D, H, W));
  EFFQ_CHECK_ARG(ws_bytes >= surf_ws(ws, P, D, H, W).bytes);
  EdtSrc src;
  src.masks = masks; src.surf = nullptr; src.C = 0;
  return edt_run<EdtVox>(src, P, D, H, W, EdtUnit{}, EdtUnit{}, EdtUnit{}, sq, as_stream(stream));
}

int effq_seg_surface(const float* logits, const uint8_t* label, int C, int D, int H, int W, int mode, int fuse,
                     float thresh, long long* counts, double* sums, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(logits && label && counts && sums && ws && C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(edt_dims_ok(2 * C, D, H, W));
  EFFQ_CHECK_ARG(mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID);
  EFFQ_CHECK_ARG(fuse == EFFQ_SEG_FUSE_NONE || fuse == EFFQ_SEG_FUSE_AGG || fuse == EFFQ_SEG_FUSE_CON);
  const int P = 2 * C;
  const size_t S = (size_t)D * H * W;
  const SurfWs s = surf_ws(ws, P, D, H, W);
  EFFQ_CHECK_ARG(ws_bytes >= s.bytes);
  const hipStream_t st = as_stream(stream);
  const long long nbins = edt_max_sq(D, H, W) + 1;
  EFFQ_HIP(hipMemsetAsync(s.hist, 0, s.hist_bytes, st));
  int rc = cc_decision_bits(logits, label, C, S, mode, fuse, thresh, s.bits, st);
  if (rc != EFFQ_OK) return rc;
  const dim3 gs(cc_grid(S, CC_STREAM_BLOCKS)), b(CC_THREADS);
  hipLaunchKernelGGL(k_surf_bits, gs, b, 0, st, s.bits, s.surf, D, H, W);
  EFFQ_LAUNCH_CHECK();
  EdtSrc src;
  src.masks = nullptr; src.surf = s.surf; src.C = C;
  rc = edt_run<EdtVox>(src, P, D, H, W, EdtUnit{}, EdtUnit{}, EdtUnit{}, s.sq, st);
  if (rc != EFFQ_OK) return rc;
  hipLaunchKernelGGL(k_surf_hist, gs, b, (size_t)P * (SURF_LOW + 1) * sizeof(uint32_t), st, s.surf, s.sq, C, (int)S, nbins,
                     s.hist);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_surf_final, dim3(C), dim3(SURF_FINAL_THREADS), 0, st, s.hist, nbins, counts, sums);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
