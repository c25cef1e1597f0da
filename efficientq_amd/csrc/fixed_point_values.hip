// The "all-values" weight fixed points: the whole project_by_iter (layer_helper.py:40-70) in ONE launch, every value
// classified on every iteration.  k_fp_small: one workgroup, the values in registers (optionally with the projection of the
// ADMM iteration as its epilogue, project_dual.h); k_fp_coop: one workgroup per CU, the values in LDS, a grid barrier per
// iteration.  admm_run.hip falls back to them for every layer that no other fixed-point family takes.
#include "common.h"
#include "fp_level.h"
#include "internal.h"
#include "project_dual.h"

namespace effq {

// ---- whole project_by_iter in ONE launch for small tensors (weights of most layers): a single
// 1024-thread workgroup computes mean|v|, then iterates statistics + update until convergence or the
// cap, all on chip.  v = a + b2 (b2 may be NULL) is formed on the fly and optionally stored to v_out.
constexpr int FPS_T = 1024;
// One barrier per iteration: every wave publishes its two partial sums into a parity-double-buffered LDS table,
// and EVERY thread adds the table in wave order and takes the division itself (same bits everywhere), so there is
// no serial thread-0 section and no broadcast barrier.  At 256 levels the weight fixed point of the first conv
// runs ~300 iterations per ADMM iteration: the per-iteration latency (2.2 us with three barriers) is what counts.
// PER = register slots per thread (compile time, so the element loop is branch-free and the fp64 chains of the
// slots interleave).
// Arithmetic per value: the level index r from the fp32 screen (fp_level.h: exact), integer tallies of r and r^2 and
// sum(r v), exact in fp64, from which level_sum_bv / _bb form sum b v and sum b^2: per value ONE fp64 multiply-add instead of
// the ~16 fp64 operations of disc64_fast + two accumulations (fp64 min/max/rint/floor issue at a fraction of the fp32
// rate; at 256 levels the first conv's weight scale takes ~290 iterations per ADMM iteration).
template <int T, int PER>
__global__ __launch_bounds__(T) void k_fp_small(const float* __restrict__ a, const float* b2, float* v_out, size_t n,
                                                effq_fp_state* st, double lo, double hi, double d, double tol,
                                                int max_iter, ProjFused pf) {
  constexpr int NW = T / 64;
  __shared__ double part[2][3][NW];
  // one workgroup on the critical path of the ADMM chain, sharing its CU with the waves of the loss conv of the previous
  // iterate: ask the issue arbiter for priority
  __builtin_amdgcn_s_setprio(3);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int kmax = (int)((n + T - 1) / T);   // live register slots (uniform)
  float vr[PER];
  unsigned live = 0;
  double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const size_t i = (size_t)tid + (size_t)k * T;
    float v = 0.0f;
    if (i < n) {
      v = (b2 != nullptr) ? (a[i] + b2[i]) : a[i];
      if (v_out != nullptr) v_out[i] = v;
      live |= 1u << k;
    }
    vr[k] = v;
    acc0 += fabs((double)v);
    acc1 += (double)v;
  }
  acc0 = wave_sum_f64_dpp(acc0);
  acc1 = wave_sum_f64_dpp(acc1);
  if (lane == 0) {
    part[0][0][wid] = acc0;
    part[0][1][wid] = acc1;
  }
  lds_barrier();
  double tot = 0.0, sv = 0.0;                // sum |v|, sum v
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    tot += part[0][0][w];
    sv += part[0][1][w];
  }
  double alpha = tot / (double)n, alpha_prev = -999.0;
  double ralpha = (double)n / tot;           // a reciprocal good to a few ulp is all the fast path needs
  double last0 = 0.0, last1 = 0.0;
  int it = 0, done = 0;
  const double rd = 1.0 / d;
  LevelConsts lc = level_grid(lo, hi, d);
  while (!done) {
    const int par = (it + 1) & 1;            // parity 0 carried the prologue sums
    lc.c1 = (float)(ralpha * rd);
    double arv = 0.0;
    int sr = 0, sr2 = 0;                     // <= 32 slots x 255^2 per thread
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      // 1024 threads leave 128 VGPRs: interleaving the chains of all 32 slots spills there, so that variant keeps a
      // (uniform) branch per slot; (a branch-free common path with the exact fallback hoisted out measured slower)
      if (T < 1024 || k < kmax) {
        const float vf = vr[k];
        const float rf = fp_level_f(vf, lc, alpha, lo, hi, d);
        const int ri = ((live >> k) & 1u) ? (int)rf : 0;      // dead slots hold v = 0: they must not count
        sr += ri;
        sr2 += ri * ri;
        arv = __builtin_fma((double)rf, (double)vf, arv);     // r v is exact in fp64 (8 + 24 bits)
      }
    }
    arv = wave_sum_f64_dpp(arv);
    const unsigned wr = group_sum_u32((unsigned)sr, 64), wr2 = group_sum_u32((unsigned)sr2, 64);
    if (lane == 0) {
      part[par][0][wid] = arv;
      part[par][1][wid] = (double)wr;
      part[par][2][wid] = (double)wr2;
    }
    lds_barrier();
    double trv = 0.0, tr = 0.0, tr2 = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      trv += part[par][0][w];
      tr += part[par][1][w];
      tr2 += part[par][2][w];
    }
    const double t0 = level_sum_bv(trv, sv, lo, d);   // sum b v
    const double t1 = level_sum_bb(tr2, tr, n, lo, d);   // sum b^2
    const double a_new = t0 / t1;
    const double ra_new = t1 / t0;           // independent of the division above (pipelines with it)
    ++it;
    fp_stop(it, max_iter, a_new, alpha, tol, done);
    alpha_prev = alpha;
    alpha = a_new;
    ralpha = ra_new;
    last0 = t0;
    last1 = t1;
  }
  if (tid == 0) fp_state_store(st, alpha, alpha_prev, last0, last1, it, done);
  if (pf.G != nullptr) {                       // the projection + dual update of this ADMM iteration, same launch
    __syncthreads();                           // v_out of every thread is in place
    proj_fused_epilogue(pf, v_out, alpha, done, tid, T);
  }
}

// ---- cooperative whole-fixed-point kernel for larger tensors --------------------------------------
// G <= 256 workgroups of 1024 threads, one per CU, each owning a contiguous slice of v that stays in LDS for
// all iterations.  Per iteration every workgroup publishes its two partial sums, all meet at a grid
// barrier, and EVERY workgroup adds the G partials in workgroup order (identical alpha everywhere, run-to-
// run and rank-to-rank deterministic -- replicated data-parallel ranks must stay bit-identical).
// Grid barrier: monotonic agent-scope counter, release fence before the arrive, relaxed polling with
// s_sleep, acquire fence after (cdna_hip_programming.md Guideline 16 / microarch "barrier-counter").
// Every spin is bounded: on time-out the state is marked done=3 and all workgroups leave.
constexpr int FPC_T = 1024;
constexpr int FPC_SLICE = 27648;          // floats per workgroup kept in LDS (108 KiB)
constexpr int FPC_MAXG = 256;          // one workgroup per CU at most: 7.08 M values = 512 x 512 x 27 weights
constexpr unsigned FPC_SPIN_LIMIT = 1u << 24;
static unsigned g_fpc_spin_limit = FPC_SPIN_LIMIT;     // effq_fp_coop_set_spin_limit (test hook)

// counter[0] = arrivals, counter[1] = check-outs, counter[2] = POISON: set by the first workgroup whose barrier times
// out.  A poisoned workspace turns every later launch into a no-op that reports done = 3 (the launches of the following
// ADMM iterations are already enqueued when a time-out happens, and the arrival counter is left non-zero by the early
// exits: they must not run on it); the host clears the workspace when it sees the error (qconv.ptq).
// INVARIANT of the exchange through fpc_barrier: whatever workgroups hand to each other across it is WRITTEN with
// fpc_publish (agent-scope atomic store: write-through, no stale line left in the writer's L2) before the barrier and
// READ with agent-scope atomic loads after it - never with plain loads: the barrier issues a release fence but NO acquire
// fence (see below), so a plain load could be served from this CU's L1.  The lock-step of data-parallel replicas rests
// on this (tests/test_configs_gpu.py: test_config2_at_its_stated_size_is_deterministic, in the default GPU selection).
__device__ __forceinline__ void fpc_publish(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool fpc_barrier(unsigned int* counter, unsigned target, int* s_fail, unsigned spin_limit) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0;
    while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(2);
      if (++spins > spin_limit ||
          __hip_atomic_load(counter + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
        __hip_atomic_store(counter + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *s_fail = 1;
        break;
      }
    }
    // No acquire fence here: everything the workgroups exchange through this barrier (the partial sums) is read with
    // agent-scope atomic loads, which are served by L2, so the L1 invalidation an acquire fence performs (buffer_inv sc1:
    // ~1.7 us per barrier, 14 barriers per call) would only protect data nobody reads; the poll above has completed
    // (its value was consumed) before any of those loads is issued.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  return *s_fail == 0;
}

template <int T>
__global__ __launch_bounds__(T) void k_fp_coop(const float* __restrict__ a, const float* __restrict__ b2,
                                                   float* __restrict__ v_out, size_t n, effq_fp_state* st, double lo,
                                                   double hi, double d, double tol, int max_iter, double* partials,
                                                   unsigned int* counter, unsigned spin_limit, FptPred* pred,
                                                   int levels) {
  __builtin_amdgcn_s_setprio(2);   // ADMM chain (critical path) over the loss / inverse streams
  // a workspace poisoned by an earlier time-out: report and leave, touching nothing (uniform across the grid: the
  // poison word only ever goes 0 -> 1 before this launch started, or during it - then the barrier below catches it)
  if (__hip_atomic_load(counter + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
    if (blockIdx.x == 0 && threadIdx.x == 0) st->done = 3;
    return;
  }

  extern __shared__ __attribute__((aligned(16))) float vs[];      // this workgroup's slice of v
  constexpr int NW = T / 64;
  __shared__ double s_wave[3][NW];
  __shared__ double s_tot[3];
  __shared__ int s_fail;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, G = gridDim.x, wg = blockIdx.x;
  const size_t per = (n + G - 1) / G;
  const size_t s0 = (size_t)wg * per, s1 = (s0 + per < n) ? s0 + per : n;
  const int cnt = (s1 > s0) ? (int)(s1 - s0) : 0;
  if (tid == 0) s_fail = 0;
  // workgroup sums of three doubles -> thread 0 (DPP wave sums, one LDS exchange; fixed tree: deterministic)
  auto wg_sum3 = [&](double& x0, double& x1, double& x2) {
    x0 = wave_sum_f64_dpp(x0);
    x1 = wave_sum_f64_dpp(x1);
    x2 = wave_sum_f64_dpp(x2);
    if (lane == 0) {
      s_wave[0][wid] = x0;
      s_wave[1][wid] = x1;
      s_wave[2][wid] = x2;
    }
    __syncthreads();
    if (tid == 0) {
      double u0 = 0.0, u1 = 0.0, u2 = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        u0 += s_wave[0][w];
        u1 += s_wave[1][w];
        u2 += s_wave[2][w];
      }
      x0 = u0;
      x1 = u1;
      x2 = u2;
    }
  };
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  for (int i = tid; i < cnt; i += T) {
    const float v = (b2 != nullptr) ? (a[s0 + i] + b2[s0 + i]) : a[s0 + i];
    if (v_out != nullptr) v_out[s0 + i] = v;
    vs[i] = v;
    acc0 += fabs((double)v);
    acc1 += (double)v;
  }
  wg_sum3(acc0, acc1, acc2);
  unsigned epoch = 0;
  // partials layout: [parity][wg][3]
  if (tid == 0) {
    fpc_publish(&partials[(0 * FPC_MAXG + wg) * 3 + 0], acc0);
    fpc_publish(&partials[(0 * FPC_MAXG + wg) * 3 + 1], acc1);
    fpc_publish(&partials[(0 * FPC_MAXG + wg) * 3 + 2], 0.0);
  }
  if (!fpc_barrier(counter, (++epoch) * (unsigned)G, &s_fail, spin_limit)) {
    if (tid == 0) st->done = 3;          // (any workgroup: workgroup 0 may have left through the poison check)
    return;
  }
  // the G partials are fetched by the lanes of wave 0 (agent-scope loads, lane l takes workgroups l, l + 64, ...) and
  // added by a fixed DPP tree: the same bits in every workgroup and run to run; the totals go to all threads through LDS
  auto combine = [&](int par, double& t0, double& t1, double& t2) {
    if (wid == 0) {
      double u0 = 0.0, u1 = 0.0, u2 = 0.0;
      for (int g = lane; g < G; g += 64) {
        u0 += __hip_atomic_load(&partials[(par * FPC_MAXG + g) * 3 + 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        u1 += __hip_atomic_load(&partials[(par * FPC_MAXG + g) * 3 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        u2 += __hip_atomic_load(&partials[(par * FPC_MAXG + g) * 3 + 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      u0 = wave_sum_f64_dpp(u0);
      u1 = wave_sum_f64_dpp(u1);
      u2 = wave_sum_f64_dpp(u2);
      if (lane == 0) {
        s_tot[0] = u0;
        s_tot[1] = u1;
        s_tot[2] = u2;
      }
    }
    __syncthreads();
    t0 = s_tot[0];
    t1 = s_tot[1];
    t2 = s_tot[2];
    __syncthreads();
  };
  double tot = 0.0, sv = 0.0, tdummy = 0.0;
  combine(0, tot, sv, tdummy);
  double alpha = tot / (double)n, alpha_prev = -999.0;
  int it = 0, done = 0;
  double last0 = 0.0, last1 = 0.0;
  // per value: level index r from the fp32 screen, then sum b v and sum b^2 from the tallies (see k_fp_small)
  const double rd = 1.0 / d;
  LevelConsts lc = level_grid(lo, hi, d);
  while (!done) {
    const int par = (it + 1) & 1;          // parity 0 was used by the abs-sum epoch
    if (wg == 0 && tid == 0) fpt_note(pred, it, alpha);      // (seeds the next call's predictions: fixed_point_traj.hip)
    lc.c1 = (float)((1.0 / alpha) * rd);
    double arv = 0.0;
    long long sr = 0, sr2 = 0;
    for (int i = tid; i < cnt; i += T) {
      const float vf = vs[i];
      const float rf = fp_level_f(vf, lc, alpha, lo, hi, d);
      const int ri = (int)rf;
      sr += ri;
      sr2 += ri * ri;
      arv = __builtin_fma((double)rf, (double)vf, arv);
    }
    double dr = (double)sr, dr2 = (double)sr2;
    wg_sum3(arv, dr, dr2);
    if (tid == 0) {
      fpc_publish(&partials[(par * FPC_MAXG + wg) * 3 + 0], arv);
      fpc_publish(&partials[(par * FPC_MAXG + wg) * 3 + 1], dr);
      fpc_publish(&partials[(par * FPC_MAXG + wg) * 3 + 2], dr2);
    }
    if (!fpc_barrier(counter, (++epoch) * (unsigned)G, &s_fail, spin_limit)) {
      if (tid == 0) st->done = 3;
      return;
    }
    double trv = 0.0, tr = 0.0, tr2 = 0.0;
    combine(par, trv, tr, tr2);
    const double t0 = level_sum_bv(trv, sv, lo, d);   // sum b v
    const double t1 = level_sum_bb(tr2, tr, n, lo, d);   // sum b^2
    const double a_new = t0 / t1;
    alpha_prev = alpha;
    ++it;
    fp_stop(it, max_iter, a_new, alpha_prev, tol, done);
    alpha = a_new;
    last0 = t0;
    last1 = t1;
  }
  if (wg == 0 && tid == 0) fp_state_finish(st, pred, alpha, alpha_prev, last0, last1, it, done, tot, levels);
  // leave the barrier counter at zero for the next launch: every workgroup is past its last poll when it gets
  // here, so the last one to check out (counter[1]) resets both words - no memset command per call.  (After a
  // barrier time-out the early returns above skip this; the host then sees done = 3 and raises.)
  if (tid == 0) {
    const unsigned left = __hip_atomic_fetch_add(counter + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (left == (unsigned)G - 1) {
      __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(counter + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ void k_check_state(const effq_fp_state* st, int32_t* err_flag) {
  if (st->done != 1) *err_flag = (st->done == 2) ? 2 : 3;
}

}  // namespace effq

using namespace effq;

extern "C" {

size_t effq_fp_small_max(void) { return (size_t)1 << 15; }

int effq_fixed_point_small(const float* a, const float* b, float* v_out, size_t n, int levels, double lo, double hi,
                           double tol, int max_iter, effq_fp_state* state_dev, void* stream) {
  return effq_fixed_point_small_fused(a, b, v_out, n, levels, lo, hi, tol, max_iter, state_dev, nullptr, stream);
}

// internal (admm_run.hip): pf != NULL runs the projection of the ADMM iteration as the kernel's epilogue
int effq_fixed_point_small_fused(const float* a, const float* b, float* v_out, size_t n, int levels, double lo, double hi,
                                 double tol, int max_iter, effq_fp_state* state_dev, const ProjFused* pf_in, void* stream) {
  ProjFused pf;
  memset(&pf, 0, sizeof(pf));
  if (pf_in != nullptr) pf = *pf_in;
  EFFQ_CHECK_ARG(pf.G == nullptr || v_out != nullptr);
  EFFQ_CHECK_ARG(a && state_dev && n > 0 && levels >= 2 && levels <= FP_LEVELS_MAX && hi > lo && max_iter > 0);
  EFFQ_CHECK_ARG(n <= effq_fp_small_max());
  EFFQ_CHECK_ARG(b == nullptr || v_out != nullptr);
  const double d = (hi - lo) / (double)(levels - 1);
  {
    // threads: 256 up to 2048 elements, 512 up to 16384 (few waves: the barrier is cheap and the element loop stays
    // short; measured best on MI355X, scripts/exp_fp256.py), else 1024; slots per thread rounded up to a power of 2
    const int T = (n <= 2048) ? 256 : (n <= 16384) ? 512 : FPS_T;
    int per = (int)((n + T - 1) / T), pp = 1;
    while (pp < per) pp <<= 1;
    hipStream_t st = as_stream(stream);
#define EFFQ_FPS(TT, PP)                                                                                          \
  hipLaunchKernelGGL((k_fp_small<TT, PP>), dim3(1), dim3(TT), 0, st, a, b, v_out, n, state_dev, lo, hi, d, tol, max_iter, pf)
    if (T == 256) {
      switch (pp) {
        case 1: EFFQ_FPS(256, 1); break;
        case 2: EFFQ_FPS(256, 2); break;
        case 4: EFFQ_FPS(256, 4); break;
        case 8: EFFQ_FPS(256, 8); break;
        case 16: EFFQ_FPS(256, 16); break;
        default: EFFQ_FPS(256, 32); break;
      }
    } else if (T == 512) {
      switch (pp) {
        case 1: case 2: case 4: EFFQ_FPS(512, 4); break;
        case 8: EFFQ_FPS(512, 8); break;
        case 16: EFFQ_FPS(512, 16); break;
        default: EFFQ_FPS(512, 32); break;
      }
    } else {
      if (pp <= 16) EFFQ_FPS(1024, 16); else EFFQ_FPS(1024, 32);
    }
#undef EFFQ_FPS
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

size_t effq_fp_coop_max(void) { return (size_t)FPC_SLICE * FPC_MAXG; }

int effq_fp_coop_set_spin_limit(unsigned int polls) {
  g_fpc_spin_limit = polls ? polls : FPC_SPIN_LIMIT;
  return EFFQ_OK;
}

int effq_fixed_point_coop(const float* a, const float* b, float* v_out, size_t n, int levels, double lo, double hi,
                          double tol, int max_iter, effq_fp_state* state_dev, void* ws, void* stream) {
  return effq_fixed_point_coop_rec(a, b, v_out, n, levels, lo, hi, tol, max_iter, state_dev, ws, nullptr, stream);
}

int effq_fixed_point_coop_rec(const float* a, const float* b, float* v_out, size_t n, int levels, double lo, double hi,
                              double tol, int max_iter, effq_fp_state* state_dev, void* ws, void* pred_dev,
                              void* stream) {
  FptPred* pred = reinterpret_cast<FptPred*>(pred_dev);
  EFFQ_CHECK_ARG(a && state_dev && ws && n > 0 && levels >= 2 && levels <= FP_LEVELS_MAX && hi > lo && max_iter > 0);
  EFFQ_CHECK_ARG(n <= effq_fp_coop_max());
  EFFQ_CHECK_ARG(b == nullptr || v_out != nullptr);
  EFFQ_CHECK_ARG(v_out == nullptr || (v_out != a && v_out != b));      // k_fp_coop's operands are __restrict__
  const double d = (hi - lo) / (double)(levels - 1);
  int G = (int)((n + FPC_SLICE - 1) / FPC_SLICE);
  if (G < 1) G = 1;
  EFFQ_CHECK_ARG(G <= FPC_MAXG);
  const size_t per = (n + G - 1) / G;
  const size_t lds = per * sizeof(float);
  // workspace: reuse the reduction workspace: partials [2][FPC_MAXG][3] doubles at its start
  double* partials = reinterpret_cast<double*>(ws);
  // the counter words sit in the tail of the reduction workspace (after the ticket), where no reduction kernel
  // writes partial sums: they must still be zero from the previous launch (the kernel leaves them at zero; the
  // reduction workspace is zero-filled at creation)
  unsigned int* counter = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(ws) +
                                                          sizeof(double) * RED_MAX_BLOCKS * RED_SLOTS + 64);
  hipStream_t st = as_stream(stream);
  int dev = 0;
  EFFQ_HIP(hipGetDevice(&dev));
  EFFQ_CHECK_ARG(dev >= 0 && dev < 64);
  // per DEVICE: the LDS attribute of the kernel and the number of workgroups that can be resident at once
  static bool known[64] = {};
  static int resident_max[64];
  if (!known[dev]) {
    EFFQ_HIP(raise_lds_limit<k_fp_coop<FPC_T>>(FPC_SLICE * sizeof(float)));
    int ncu = 0, per_cu = 0;
    EFFQ_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    EFFQ_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_fp_coop<FPC_T>, FPC_T, FPC_SLICE * sizeof(float)));
    resident_max[dev] = ncu * per_cu;
    known[dev] = true;
  }
  // The grid barrier needs every workgroup resident at once.  That holds on a whole MI355X (G <= 256 = its CU count,
  // one workgroup per CU by LDS; workgroups of other streams only delay a late arrival: they retire, they never wait
  // for this kernel); on a partitioned device (CPX / DPX) or a smaller part it may not: then the fixed point runs as one
  // launch per iteration (each a no-op once converged) - slower, never stuck.
  if (G > resident_max[dev]) {
    int rc = (b != nullptr) ? effq_admm_presum(a, b, v_out, n, stream) : EFFQ_OK;
    const float* src = (b != nullptr) ? v_out : a;
    double* s0 = red_ws(ws).partials + (size_t)RED_MAX_BLOCKS * (RED_SLOTS - 1);   // two spare doubles of the workspace
    if (rc == EFFQ_OK) rc = effq_abs_sum_f64(src, n, s0, ws, stream);
    if (rc == EFFQ_OK) rc = effq_fp_init(state_dev, s0, stream);
    if (rc == EFFQ_OK) rc = effq_alpha_fixed_point(src, n, levels, lo, hi, tol, max_iter, max_iter, state_dev, ws, stream);
    return rc;
  }
  hipLaunchKernelGGL(k_fp_coop<FPC_T>, dim3(G), dim3(FPC_T), lds, st, a, b, v_out, n, state_dev, lo, hi, d, tol,
                     max_iter, partials, counter, g_fpc_spin_limit, pred, levels);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_fp_check(const effq_fp_state* state_dev, int32_t* err_flag_dev, void* stream) {
  EFFQ_CHECK_ARG(state_dev && err_flag_dev);
  hipLaunchKernelGGL(k_check_state, dim3(1), dim3(1), 0, as_stream(stream), state_dev, err_flag_dev);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
