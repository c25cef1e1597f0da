// Shared host/device helpers for the effq HIP library (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/effq_hip.h"

namespace effq {

void set_error(const char* fmt, ...);

#define EFFQ_CHECK_ARG(cond)                                                        \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      effq::set_error("%s:%d: argument check failed: %s", __FILE__, __LINE__, #cond); \
      return EFFQ_ERR_ARG;                                                          \
    }                                                                               \
  } while (0)

#define EFFQ_HIP(call)                                                                   \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess) {                                                              \
      effq::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
      return EFFQ_ERR_HIP;                                                               \
    }                                                                                    \
  } while (0)

#define EFFQ_LAUNCH_CHECK() EFFQ_HIP(hipGetLastError())

// the caller's workspace against what the entry point needs; the message names the entry point
#define EFFQ_CHECK_WS(have, need)                                                                          \
  do {                                                                                                     \
    if ((have) < (need)) {                                                                                 \
      effq::set_error("%s: workspace of %zu bytes, needs %zu", __func__, (size_t)(have), (size_t)(need)); \
      return EFFQ_ERR_WORKSPACE;                                                                           \
    }                                                                                                      \
  } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Raises KERNEL's dynamic-LDS limit on the current device to at least `bytes`.  The attribute belongs to the device, so
// the record of what was set is kept per device (hipGetDevice): a fixed size is set once per device, a varying one again
// only when a launch needs more than was set.  Use as EFFQ_HIP(raise_lds_limit<kernel>(bytes)).
template <auto KERNEL>
static inline hipError_t raise_lds_limit(size_t bytes) {
  constexpr int MAX_DEV = 64;
  static size_t set[MAX_DEV] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= MAX_DEV) return hipErrorInvalidDevice;
  if (bytes > set[dev]) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)bytes);
    if (e != hipSuccess) return e;
    set[dev] = bytes;
  }
  return hipSuccess;
}

// Profiling ablations ("run the kernel without its MFMA loop / its loads ...") exist only in builds made with
// -DEFFQ_ABLATE (make ABLATE=1): in the shipped library EFFQ_DBG(p) is the constant 0 and the branches fold away, and no
// environment variable is read on a launch path.
#ifdef EFFQ_ABLATE
#define EFFQ_DBG(p) ((p).debug)
static inline int effq_ablate_env(const char* name) {
  const char* v = getenv(name);
  return v ? atoi(v) : 0;
}
#else
#define EFFQ_DBG(p) 0
static inline int effq_ablate_env(const char*) { return 0; }
#endif

// ---- reduction workspace -------------------------------------------------------------
// [0, RED_MAX_BLOCKS*RED_SLOTS) doubles of per-block partials, then one uint32 ticket.
constexpr int RED_MAX_BLOCKS = 2048;
constexpr int RED_SLOTS = 4;
constexpr size_t RED_WS_BYTES = sizeof(double) * RED_MAX_BLOCKS * RED_SLOTS + 256;

struct RedWs {
  double* partials;
  unsigned int* ticket;
};
static inline RedWs red_ws(void* ws) {
  RedWs r;
  r.partials = reinterpret_cast<double*>(ws);
  r.ticket = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(ws) +
                                             sizeof(double) * RED_MAX_BLOCKS * RED_SLOTS);
  return r;
}

// The streaming kernels (quant_reduce.hip, project_dual.hip): TPB threads, grid-stride over at most RED_MAX_BLOCKS blocks.
constexpr int TPB = 256;
static inline int stream_grid(size_t n_vec) {
  size_t b = (n_vec + TPB - 1) / TPB;
  if (b < 1) b = 1;
  if (b > RED_MAX_BLOCKS) b = RED_MAX_BLOCKS;
  return (int)b;
}

#ifdef __HIPCC__
// Workgroup barrier that orders LDS traffic only.  __syncthreads() is a fence + barrier and the fence waits for
// vmcnt(0): every global load in flight - i.e. the register prefetch of the NEXT tile - is drained at each barrier
// (cdna_hip_programming.md, "Pipelining across barriers").  Tiles are handed over through LDS and registers only, so
// the LDS counter is all the barrier needs: s_waitcnt lgkmcnt(0) (0xC07F: vmcnt and expcnt left alone) + s_barrier.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// 64-lane wave sum, __shfl_down: ONLY LANE 0 holds the total, lanes 1 to 63 end with partial sums.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// 64-lane wave sum, xor butterfly: every lane ends with the total; the same tree in every lane.
__device__ __forceinline__ uint32_t wave_sum_all(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum_all(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_all(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Equal keys of a wave are added once: one key per valid lane, and the lanes that hold the same key as the first lane
// still to do form a group (ballot, leader, popcount), for at most ROUNDS groups.  Returns what this lane must add at its
// key: the group's count in the group's leader, 1 in a lane left over after the rounds (more distinct keys than rounds:
// one add per lane), 0 elsewhere.  Every lane of the wave calls it (the ballots need them all).  group(m, leader) is
// called once per round with the lane mask of the round's group and whether this lane leads it; false ends the rounds.
struct WaveMatchEvery {
  __device__ __forceinline__ bool operator()(unsigned long long, bool) const { return true; }
};
template <int ROUNDS, typename F = WaveMatchEvery>
__device__ __forceinline__ uint32_t wave_match_count(bool valid, uint32_t key, int lane, F group = F{}) {
  unsigned long long todo = __ballot(valid);
  uint32_t add = 0;                                       // the leader of a group carries the group's count
  for (int round = 0; round < ROUNDS && todo; ++round) {
    const int lead = __ffsll((long long)todo) - 1;
    const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, lead);
    const unsigned long long m = __ballot(key == k) & todo;
    if (lane == lead) add = (uint32_t)__popcll(m);
    todo &= ~m;
    if (!group(m, lane == lead)) break;
  }
  if ((todo >> lane) & 1ull) add = 1;
  return add;
}

// ---- DPP reductions over groups of GS lanes (GS a power of two <= 64); every lane of a 16-lane row ends with the
// row's total, groups of 32 / 64 are finished with readlane.  Fixed tree: deterministic for fp64 too.
// INVARIANT: every lane of a group that enters the tree must be active (for wave_sum_f64_dpp and gs = 64: all 64
// lanes; for smaller groups: whole, aligned groups - a wave may have some groups switched off, never part of one).
// A DPP move whose source lane is switched off in EXEC returns `old` (0 here), so the partial sums that lane should have
// carried through the xor / mirror butterfly are lost to every lane that reads from it.  The removed sorted-value fixed
// point (round 3: "wrong totals at one boundary per lane, right totals with four boundary slots per lane or an
// unconditional re-sum") is that pattern: the variants that gave right totals are exactly those that entered the tree
// with all 64 lanes.  The call sites of this library: whole waves (operands of absent elements set to 0, not their
// lanes switched off), or - fpb_iterate - groups of gs lanes that are active or inactive as a whole.
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = dpp_u32<CTRL>((unsigned)u), hi = dpp_u32<CTRL>((unsigned)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;

__device__ __forceinline__ unsigned group_sum_u32(unsigned v, int gs) {
  if (gs >= 2) v += dpp_u32<DPP_XOR1>(v);
  if (gs >= 4) v += dpp_u32<DPP_XOR2>(v);
  if (gs >= 8) v += dpp_u32<DPP_HALF_MIRROR>(v);
  if (gs >= 16) v += dpp_u32<DPP_MIRROR>(v);
  if (gs >= 32) {
    const int lane = threadIdx.x & 63;
    const unsigned r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16),
                   r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    if (gs == 32)
      v = (lane < 32) ? r0 + r1 : r2 + r3;
    else
      v = (r0 + r1) + (r2 + r3);
  }
  return v;
}
__device__ __forceinline__ double wave_sum_f64_dpp(double v) {
  v += dpp_f64<DPP_XOR1>(v);
  v += dpp_f64<DPP_XOR2>(v);
  v += dpp_f64<DPP_HALF_MIRROR>(v);
  v += dpp_f64<DPP_MIRROR>(v);
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  double r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, 16 * i), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), 16 * i);
    r[i] = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
  }
  return (r[0] + r[1]) + (r[2] + r[3]);
}

// Block-wide sum of NS doubles per thread; result valid in thread 0.  smem: NS*16 doubles.
template <int NS>
__device__ __forceinline__ void block_sum(double (&v)[NS], double* smem) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int s = 0; s < NS; ++s) v[s] = wave_sum(v[s]);
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < NS; ++s) smem[s * 16 + wid] = v[s];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      double t = 0.0;
      for (int w = 0; w < nw; ++w) t += smem[s * 16 + w];
      v[s] = t;
    }
  }
  __syncthreads();
}

// Grid-wide deterministic sum: every block publishes NS partials, the block that draws the last
// ticket adds all partials in block order and writes out[0..NS).  Inter-workgroup hand-off follows
// the agent-scope release/acquire recipe (cdna_hip_programming.md, Guideline 16): plain stores by
// one lane -> release fence -> vmcnt(0) -> relaxed agent ticket; last block: acquire fence ->
// vmcnt(0) -> barrier -> loads.  The ticket is reset by the last block (ws zeroed once at creation).
template <int NS>
__device__ __forceinline__ void grid_sum_finish(double (&v)[NS], double* partials, unsigned int* ticket,
                                                double* out, double* smem, int* s_last,
                                                unsigned int bid = blockIdx.x, unsigned int nblk = gridDim.x) {
  block_sum<NS>(v, smem);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < NS; ++s) partials[(size_t)bid * NS + s] = v[s];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = (t == nblk - 1) ? 1 : 0;
  }
  __syncthreads();
  if (*s_last) {
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
    // fixed assignment of partials to threads + fixed tree => run-to-run deterministic
    for (unsigned int b = threadIdx.x; b < nblk; b += blockDim.x) {
#pragma unroll
      for (int s = 0; s < NS; ++s)
        acc[s] += __hip_atomic_load(&partials[(size_t)b * NS + s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    block_sum<NS>(acc, smem);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int s = 0; s < NS; ++s) out[s] = acc[s];
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
#endif  // __HIPCC__

}  // namespace effq
