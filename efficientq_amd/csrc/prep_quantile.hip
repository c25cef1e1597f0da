// Exact order statistics of a subject's modalities on the device, for the percentile window of the `prep` mission
// (prep.py, --prep_window pLO,pHI, where the rule is defined), and the masked window that applies the bounds.
//
// effq_prep_quantiles: x (C, S) fp32; per modality c the n voxels of its own mask, sorted ascending by the
// order-preserving 32-bit key of the float (pq_key: -0.0 counts as +0.0, every NaN comes after +Inf), and per percentile
// q_r the two order statistics sorted[k] and sorted[min(k + 1, n - 1)], k = floor((n - 1) q_r / 100) in fp64 with the
// product first.  A radix select, most significant digit first, 8 bits in four passes:
//   k_pq_hist    streams x once per pass (blockIdx.y = the modality) and counts, per prefix that is still followed, the
//                next digit of the voxels whose key starts with that prefix: 32-bit counters in LDS, 256 per prefix, at
//                most 2 R <= 8 prefixes (8 KB), added to the pass's counters in `ws` by integer atomics at the end;
//   k_pq_select  one workgroup, one wave per modality: per target a wave scan over the 256 counters of its prefix finds
//                the digit that holds the target's rank and the rank that remains inside it.  Targets whose prefixes are
//                equal share one set of counters in the next pass (the two statistics of a percentile nearly always do).
// Pass 0 follows the empty prefix: its counters also give n, from which the select step forms the ranks.  After pass 3
// a prefix is the key of the statistic itself.  n = 0: no prefix is followed, both statistics are NaN.
// Eight bits and not 11 / 11 / 10: with up to eight prefixes followed at once the wider digits need 64 KB of LDS per
// workgroup (one workgroup per CU where 8 KB lets eight stay resident to hide the load latency), and each of the 1024
// workgroups would clear and flush up to 16384 counters per pass, which is the traffic of a further pass.
// Heavy ties (the air of a CT scan, a zero background under MASK_ALL) put most of a wave into one counter: equal
// counters of a wave are combined by ballot before the LDS atomic (pq_add, the scheme of seg_sweep.hip); the rounds end
// early once one combines only a few lanes, since a digit of mantissa bits spreads a wave over as many counters.
// Loads as in prep.hip: 16 B through the 4-B-aligned PFloat4, the last S % 4 voxels one by one by the first wave of
// workgroup 0.  Nine launches on `stream` (one that clears the counters, four pairs), no read by the host, no workgroup
// that waits for another, integer atomics only: equal inputs give equal bits.
//
// effq_prep_mask_window: x[i] = in_mask(x[i]) ? clip(x[i]) : x[i] in place, clip that of effq_prep_window.
#include <math.h>
#include "common.h"
#include "prep_rows.h"

namespace effq {

constexpr int PQ_MAXC = EFFQ_PREP_MAX_MODALITIES;
constexpr int PQ_TARGETS = 2 * EFFQ_PREP_QUANTILE_MAX;      // order statistics followed per modality
constexpr int PQ_BINS = 256;
constexpr int PQ_PASSES = 4;
constexpr int PQ_MATCH_ROUNDS = 4;                          // distinct counters of a wave that are combined by ballot
constexpr int PQ_MATCH_MIN = 8;                             // a round that combined fewer lanes than this is the last
constexpr int PQ_HIST_WORDS = PQ_PASSES * PQ_MAXC * PQ_TARGETS * PQ_BINS;
static_assert(PQ_MAXC <= PREP_WAVES, "k_pq_select: one wave per modality");
static_assert(PQ_BINS == 4 * 64, "k_pq_select: four counters per lane");

struct PqState {              // of one modality, between the passes
  uint32_t n;                 // voxels inside the mask
  uint32_t nu;                // distinct prefixes followed in the next pass; 0: nothing to follow
  uint32_t uprefix[PQ_TARGETS];
  uint32_t prefix[PQ_TARGETS], rank[PQ_TARGETS], slot[PQ_TARGETS];    // per target; slot: which of uprefix it has
};
constexpr size_t PQ_WS_BYTES = sizeof(uint32_t) * PQ_HIST_WORDS + sizeof(PqState) * PQ_MAXC;

struct PqWs {
  uint32_t* hist;             // (PQ_PASSES, PQ_MAXC, PQ_TARGETS, PQ_BINS)
  PqState* state;             // (PQ_MAXC)
};
static inline PqWs pq_ws(void* ws) {
  PqWs r;
  r.hist = static_cast<uint32_t*>(ws);
  r.state = reinterpret_cast<PqState*>(r.hist + PQ_HIST_WORDS);
  return r;
}
struct PqQ {
  double q[EFFQ_PREP_QUANTILE_MAX];
};

// ascending keys = ascending floats; -0.0 is +0.0, every NaN is the last key
__device__ __forceinline__ uint32_t pq_key(float v) {
  if (v != v) return 0xffffffffu;
  if (v == 0.0f) return 0x80000000u;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pq_value(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// adds one to counter `k` of s_hist per valid lane; every lane of the wave calls it (the ballots need them all)
__device__ __forceinline__ void pq_add(uint32_t* s_hist, bool valid, uint32_t k, int lane) {
  // a small group ends the rounds: the digits are spread (mantissa bits), ballots do not pay
  const uint32_t add = wave_match_count<PQ_MATCH_ROUNDS>(
      valid, k, lane, [](unsigned long long m, bool) { return __popcll(m) >= PQ_MATCH_MIN; });
  if (add) atomicAdd(&s_hist[k], add);
}

struct PqFollow {
  uint32_t up[PQ_TARGETS];
  int nu, pass;
  int mask_mode;
};

// one voxel: inside the mask and under a followed prefix, its next digit is counted
__device__ __forceinline__ void pq_voxel(uint32_t* s_hist, const PqFollow& f, bool valid, float v, int lane) {
  const uint32_t key = pq_key(v);
  const int shift = 32 - 8 * f.pass;                      // the bits of the prefix: key >> shift
  uint32_t slot = 0;
  bool found = f.pass == 0;
  if (f.pass != 0) {
    const uint32_t hi = key >> shift;
#pragma unroll
    for (int j = 0; j < PQ_TARGETS; ++j)
      if (j < f.nu && hi == f.up[j]) { slot = j; found = true; }
  }
  const uint32_t digit = (key >> (shift - 8)) & 0xffu;
  pq_add(s_hist, valid && found && in_mask(v, f.mask_mode), slot * PQ_BINS + digit, lane);
}

__global__ __launch_bounds__(PREP_THREADS) void k_pq_clear(uint32_t* __restrict__ hist) {
  for (unsigned i = blockIdx.x * PREP_THREADS + threadIdx.x; i < (unsigned)PQ_HIST_WORDS; i += gridDim.x * PREP_THREADS)
    hist[i] = 0;
}

__global__ __launch_bounds__(PREP_THREADS) void k_pq_hist(const float* __restrict__ x, unsigned S, int mask_mode, int pass,
                                                          PqWs ws) {
  __shared__ uint32_t s_hist[PQ_TARGETS * PQ_BINS];
  const int c = blockIdx.y;
  const PqState* st = ws.state + c;
  PqFollow f;
  f.pass = pass;
  f.mask_mode = mask_mode;
  f.nu = pass == 0 ? 1 : (int)min(st->nu, (uint32_t)PQ_TARGETS);      // the same for the whole workgroup
  if (f.nu == 0) return;
#pragma unroll
  for (int j = 0; j < PQ_TARGETS; ++j) f.up[j] = (pass != 0 && j < f.nu) ? st->uprefix[j] : 0u;
  const int used = f.nu * PQ_BINS;
  for (int k = threadIdx.x; k < used; k += PREP_THREADS) s_hist[k] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const float* xc = x + (size_t)c * S;
  const unsigned groups = S / 4;
  // the trip count is the same for every lane of the workgroup: the ballots need whole waves
  // and the next trip's load is issued before this trip's voxels are counted
  const unsigned stride = gridDim.x * PREP_THREADS, first = blockIdx.x * PREP_THREADS + threadIdx.x;
  PFloat4 next;
  next.x = next.y = next.z = next.w = 0.0f;
  if (first < groups) next = *reinterpret_cast<const PFloat4*>(xc + (size_t)first * 4);
  for (unsigned g0 = blockIdx.x * PREP_THREADS; g0 < groups; g0 += stride) {
    const unsigned g = g0 + threadIdx.x;
    const bool valid = g < groups;
    const PFloat4 v4 = next;
    if (g + stride < groups) next = *reinterpret_cast<const PFloat4*>(xc + (size_t)(g + stride) * 4);
    pq_voxel(s_hist, f, valid, v4.x, lane);
    pq_voxel(s_hist, f, valid, v4.y, lane);
    pq_voxel(s_hist, f, valid, v4.z, lane);
    pq_voxel(s_hist, f, valid, v4.w, lane);
  }
  // the last S % 4 voxels: the first wave of workgroup 0, a lane each
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const unsigned t = groups * 4 + threadIdx.x;
    const bool valid = t < S;
    pq_voxel(s_hist, f, valid, valid ? xc[t] : 0.0f, lane);
  }
  __syncthreads();
  uint32_t* out = ws.hist + ((size_t)pass * PQ_MAXC + c) * PQ_TARGETS * PQ_BINS;
  for (int k = threadIdx.x; k < used; k += PREP_THREADS) {
    const uint32_t n = s_hist[k];
    if (n) atomicAdd(&out[k], n);
  }
}

__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v, int lane) {      // inclusive
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// One workgroup; wave c takes modality c.  No barrier: the waves share nothing.
__global__ __launch_bounds__(PREP_THREADS) void k_pq_select(PqWs ws, int C, int R, PqQ q, int pass,
                                                            long long* __restrict__ count_out,
                                                            float* __restrict__ stat_out) {
  const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
  if (c >= C) return;
  PqState* st = ws.state + c;
  const uint32_t* hist = ws.hist + ((size_t)pass * PQ_MAXC + c) * PQ_TARGETS * PQ_BINS;
  const int T = 2 * R;
  uint32_t n, prefix[PQ_TARGETS], rank[PQ_TARGETS], slot[PQ_TARGETS];
  if (pass == 0) {
    n = wave_sum_all(hist[4 * lane] + hist[4 * lane + 1] + hist[4 * lane + 2] + hist[4 * lane + 3]);
#pragma unroll
    for (int t = 0; t < PQ_TARGETS; ++t) {
      uint32_t k = 0;
      if (t < T && n > 0) {
        const double h = (double)(n - 1) * q.q[t >> 1] / 100.0;      // the product first (prep.percentile_value)
        k = (uint32_t)floor(h);
        if (t & 1) k = k + 1 < n ? k + 1 : n - 1;
      }
      prefix[t] = 0; rank[t] = k; slot[t] = 0;
    }
  } else {
    n = st->n;
#pragma unroll
    for (int t = 0; t < PQ_TARGETS; ++t) {
      prefix[t] = st->prefix[t]; rank[t] = st->rank[t]; slot[t] = st->slot[t] & (PQ_TARGETS - 1);
    }
  }
  if (n == 0) {               // an empty mask: nothing is followed
    if (lane == 0) {
      if (pass == 0) { st->n = 0; st->nu = 0; }
      if (pass == PQ_PASSES - 1) {
        count_out[c] = 0;
        for (int t = 0; t < T; ++t) stat_out[(size_t)c * T + t] = __uint_as_float(0x7fc00000u);
      }
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < PQ_TARGETS; ++t) {
    if (t < T) {
      const uint32_t* h = hist + slot[t] * PQ_BINS + 4 * lane;
      const uint32_t b0 = h[0], b1 = h[1], b2 = h[2], b3 = h[3];
      const uint32_t own = b0 + b1 + b2 + b3;
      const uint32_t incl = wave_scan_u32(own, lane), excl = incl - own;
      const unsigned long long hit = __ballot(rank[t] >= excl && rank[t] < incl);
      const int lead = hit ? __ffsll((long long)hit) - 1 : 63;      // exactly one lane: rank < the counters' total
      uint32_t r = rank[t] - excl, d = 0;
      if (r >= b0) { r -= b0; d = 1;
        if (r >= b1) { r -= b1; d = 2;
          if (r >= b2) { r -= b2; d = 3; } } }
      const uint32_t digit = (uint32_t)__shfl((int)(4 * lane + d), lead, 64);
      rank[t] = (uint32_t)__shfl((int)r, lead, 64);
      prefix[t] = (prefix[t] << 8) | digit;
    }
  }
  // targets with equal prefixes share the counters of the next pass
  uint32_t up[PQ_TARGETS];
  int nu = 0;
#pragma unroll
  for (int t = 0; t < PQ_TARGETS; ++t) up[t] = 0;
#pragma unroll
  for (int t = 0; t < PQ_TARGETS; ++t) {
    if (t < T) {
      int j = 0;
      while (j < nu && up[j] != prefix[t]) ++j;
      if (j == nu) up[nu++] = prefix[t];
      slot[t] = (uint32_t)j;
    }
  }
  if (lane == 0) {
    if (pass < PQ_PASSES - 1) {
      st->n = n;
      st->nu = (uint32_t)nu;
      for (int t = 0; t < PQ_TARGETS; ++t) {
        st->uprefix[t] = up[t]; st->prefix[t] = prefix[t]; st->rank[t] = rank[t]; st->slot[t] = slot[t];
      }
    } else {                  // the prefix is the whole key
      count_out[c] = (long long)n;
      for (int t = 0; t < T; ++t) stat_out[(size_t)c * T + t] = pq_value(prefix[t]);
    }
  }
}

__global__ __launch_bounds__(PREP_THREADS) void k_prep_mask_window(float* __restrict__ x, size_t n, float lo, float hi,
                                                                   int mask_mode) {
  auto clip = [&](float v) {      // numpy.clip inside the mask: a NaN stays a NaN
    return in_mask(v, mask_mode) ? (v < lo ? lo : (v > hi ? hi : v)) : v;
  };
  const size_t groups = n / 4;
  for (size_t g = (size_t)blockIdx.x * PREP_THREADS + threadIdx.x; g < groups; g += (size_t)gridDim.x * PREP_THREADS) {
    PFloat4 v = *reinterpret_cast<const PFloat4*>(x + g * 4);
    v.x = clip(v.x); v.y = clip(v.y); v.z = clip(v.z); v.w = clip(v.w);
    *reinterpret_cast<PFloat4*>(x + g * 4) = v;
  }
  const size_t t = groups * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) x[t] = clip(x[t]);
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_prep_quantile_ws_bytes(size_t* bytes) {
  EFFQ_CHECK_ARG(bytes);
  *bytes = PQ_WS_BYTES;
  return EFFQ_OK;
}

int effq_prep_quantiles(const float* x, int C, long long S, int mask_mode, const double* q, int R, long long* count_out,
                        float* stat_out, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(x && q && count_out && stat_out && ws && C <= PQ_MAXC && prep_fits_flat(C, S));
  EFFQ_CHECK_ARG(mask_mode == EFFQ_PREP_MASK_NONZERO || mask_mode == EFFQ_PREP_MASK_ALL);
  EFFQ_CHECK_ARG(R >= 1 && R <= EFFQ_PREP_QUANTILE_MAX);
  EFFQ_CHECK_ARG(ws_bytes >= PQ_WS_BYTES && aligned_to(x, 4) && aligned_to(ws, 8) && aligned_to(count_out, 8) &&
                 aligned_to(stat_out, 4));
  PqQ pq;
  for (int r = 0; r < EFFQ_PREP_QUANTILE_MAX; ++r) {
    pq.q[r] = r < R ? q[r] : 0.0;
    EFFQ_CHECK_ARG(pq.q[r] >= 0.0 && pq.q[r] <= 100.0);       // false for a NaN
  }
  const PqWs w = pq_ws(ws);
  const hipStream_t st = as_stream(stream);
  const dim3 g(prep_grid((size_t)S / 4), C), t(PREP_THREADS);
  hipLaunchKernelGGL(k_pq_clear, dim3(PQ_HIST_WORDS / PREP_THREADS / 4), t, 0, st, w.hist);
  EFFQ_LAUNCH_CHECK();
  for (int pass = 0; pass < PQ_PASSES; ++pass) {
    hipLaunchKernelGGL(k_pq_hist, g, t, 0, st, x, (unsigned)S, mask_mode, pass, w);
    EFFQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pq_select, dim3(1), t, 0, st, w, C, R, pq, pass, count_out, stat_out);
    EFFQ_LAUNCH_CHECK();
  }
  return EFFQ_OK;
}

int effq_prep_mask_window(float* x, size_t n, float lo, float hi, int mask_mode, void* stream) {
  EFFQ_CHECK_ARG(x && n > 0 && aligned_to(x, 4) && lo <= hi);       // a NaN bound fails lo <= hi
  EFFQ_CHECK_ARG(mask_mode == EFFQ_PREP_MASK_NONZERO || mask_mode == EFFQ_PREP_MASK_ALL);
  hipLaunchKernelGGL(k_prep_mask_window, dim3(prep_grid(n / 4)), dim3(PREP_THREADS), 0, as_stream(stream), x, n, lo, hi,
                     mask_mode);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
