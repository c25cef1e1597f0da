// The quantiser arithmetic every fixed-point family must agree on bit for bit: the level index of the reference
// (layer_helper.py:25-37 evaluated in fp64) with its fp32 screen, the scale sums from integer level tallies, the stop
// rule of project_by_iter (layer_helper.py:55-64) and the final state store.  The kernels (quant_reduce.hip,
// project_dual.{h,hip}, fixed_point_{values,bucket,bracket,channels}.hip, fp_traj.h) keep their own loops and reductions around them.
#pragma once
#include <math.h>
#include "common.h"

namespace effq {

// Exact level index of x at scale a: the reference's own arithmetic (IEEE fp64 divisions, round-half-even).
__device__ __forceinline__ double level_exact(double x, double a, double lo, double hi, double d) {
  double t = x / a;
  t = fmin(fmax(t, lo), hi);
  return rint((t - lo) / d);
}
// discretize (layer_helper.py:25-37) in fp64: the exact level and its value r d + lo
__device__ __forceinline__ double disc64(double x, double alpha, double lo, double hi, double d, double* idx) {
  const double r = level_exact(x, alpha, lo, hi, d);
  *idx = r;
  return r * d + lo;
}
// (not inlined: the fallback of the screen is taken for ~4 values in 10 000, and its two IEEE divisions are ~100
// instructions that would otherwise be copied into every unrolled call site)
__device__ __attribute__((noinline)) inline int fp_level_exact(float v, double a, double lo, double hi, double d) {
  return (int)level_exact((double)v, a, lo, hi, d);
}

// Screen constants: u = v c1 + c0 is (v / a - lo) / d in fp32, clamped to [0, lmax].  level_consts derives c1 from 1/a;
// kernels that derive it otherwise (from sum b^2 / sum bv, or per bracket end) start from level_grid and set c1.
struct LevelConsts {
  float c1, c0, lmax;
};
__device__ __forceinline__ LevelConsts level_consts(double a, double lo, double hi, double d) {
  LevelConsts c;
  const double rd = 1.0 / d;
  c.c1 = (float)((1.0 / a) * rd);
  c.c0 = (float)(-lo * rd);
  c.lmax = (float)rint((hi - lo) * rd);
  return c;
}
__device__ __forceinline__ LevelConsts level_grid(double lo, double hi, double d) {
  LevelConsts c;
  const double rd = 1.0 / d;
  c.c1 = 0.0f;
  c.c0 = (float)(-lo * rd);
  c.lmax = (float)rint((hi - lo) * rd);
  return c;
}

// The fp32 screen: u is off by <= 1.5 lmax 2^-24 (c1 rounded to fp32 on a product of <= lmax / 2, the fma's own rounding
// of <= lmax 2^-24; c0 is exact) = 2.3e-5 at 256 levels, so rint(u) is the exact level unless u lies within 2e-4 of a
// rounding boundary.  Returns false there: the caller's exact arithmetic decides.  A NaN does NOT fail the screen: a NaN v
// (or a NaN c1) makes u NaN, fmaxf(NaN, 0) is 0 and level 0 is accepted - the level level_exact gives it too, its fmax
// dropping the NaN of v / a the same way.  A NaN value is not lost for that: level_accum of quant_reduce.hip adds
// fma(0, NaN) to its sum of r v, which is then NaN, and the scale update ends NaN with done = 1, as the reference's loop
// does (tests/test_quant_reduce_gpu.py).
// The band is a constant, so
// the bound on u must stay well inside it: every entry point that gets here refuses levels > FP_LEVELS_MAX (the bound
// reaches the band near 2200 levels; emulated in numpy at 65536 levels, the screen puts 4 in 1000 of the values next to
// a boundary on the wrong level).
constexpr int FP_LEVELS_MAX = 256;
__device__ __forceinline__ bool level_screen(float v, const LevelConsts& c, float& rf) {
  float u = __builtin_fmaf(v, c.c1, c.c0);
  u = fminf(fmaxf(u, 0.0f), c.lmax);
  rf = rintf(u);
  return fabsf(u - rf) < 0.4998f;
}
// Screened level of v at scale a (the scale c was built for), the exact fallback inline ...
__device__ __forceinline__ float fp_level_f(float v, const LevelConsts& c, double a, double lo, double hi, double d) {
  float rf;
  if (!level_screen(v, c, rf)) rf = (float)level_exact((double)v, a, lo, hi, d);
  return rf;
}
// ... or out of line (fp_level_exact)
__device__ __forceinline__ int fp_level(float v, const LevelConsts& c, double a, double lo, double hi, double d) {
  float rf;
  if (!level_screen(v, c, rf)) return fp_level_exact(v, a, lo, hi, d);
  return (int)rf;
}

// Scale sums of n values from their level tallies: b = r d + lo depends on the level r alone, so
//   sum b v = d sum(r v) + lo sum(v),   sum b^2 = d^2 sum(r^2) + 2 d lo sum(r) + lo^2 n
// with sum(r), sum(r^2) exact integers and r v exact in fp64.
__device__ __forceinline__ double level_sum_bv(double srv, double sv, double lo, double d) { return d * srv + lo * sv; }
template <class N>   // (the count in its caller's type: converted where the formula uses it)
__device__ __forceinline__ double level_sum_bb(double sr2, double sr, N n, double lo, double d) {
  const double lo2n = lo * lo * (double)n;
  return (d * d * sr2 + 2.0 * d * lo * sr) + lo2n;
}

// Stop rule of project_by_iter after step `it` (counted from 1) moved the scale from alpha to a_new: done = 2 at the cap
// (the reference raises whenever c == max_iter, even if that last step converged: layer_helper.py:62-64), else done = 1
// once |a_new - alpha| <= tol (or is NaN); otherwise done is left as it is (0 while iterating).
__device__ __forceinline__ void fp_stop(int it, int max_iter, double a_new, double alpha, double tol, int& done) {
  if (it >= max_iter)
    done = 2;
  else if (!(fabs(a_new - alpha) > tol))
    done = 1;
}

// ---- prediction of a fixed point's iterates from the previous call on (nearly) the same tensor -----------------------
// The weight projection of ADMM iteration k runs project_by_iter on v_k = w*_k + dual_{k-1}, which differs little from
// v_{k-1}: the i-th iterate of call k lies within ~1e-3 (early) ... 1e-9 (late) of the i-th iterate of call k - 1.
// Slots 0 .. FPT_SLOTS-2 hold one iterate each, the last slot the hull of all later ones and of the final scale.
constexpr int FPT_SLOTS = 8;
struct FptPred {
  int K;                      // valid slots (0 = nothing known: cold)
  int e;                      // exponent of the integer unit the tallies of the next call use (q = 2^-e)
  int e_valid, pad;
  double lo[FPT_SLOTS], hi[FPT_SLOTS];      // the iterate (lo = hi), or the hull of the tail
  double eps[FPT_SLOTS];                    // relative margin of the WIDE bracket around it (envelope of the recent drifts)
  double nlo[FPT_SLOTS], nhi[FPT_SLOTS];    // the same of the call in progress (becomes lo / hi at its end)
  long long calls, warm_iters, full_iters, listed, list_max;      // diagnostics
  double eps_n[FPT_SLOTS];                  // margin of the NARROW bracket (follows the last drift closely), <= eps
  long long ring_iters, ring_listed;        // diagnostics: iterates served by the wide bracket, entries of its list
  long long trace[8];                       // diagnostics: 100 MHz time stamps of the last workgroup of the last call
};
constexpr double FPT_EPS_MIN = 1e-4, FPT_EPS_MAX = 0.03, FPT_EPS_NEW = 0.01;

// Recorder, used by whichever kernel runs the fixed point: fpt_note(i, alpha_i) by ONE thread for every classification
// scale in order; then, after a barrier (or by the same thread), fpt_finish_slot for j = 0 .. FPT_SLOTS-1 (any threads)
// and fpt_finish_head once.  pred == nullptr: nothing is recorded.
__device__ __forceinline__ void fpt_note(FptPred* p, int i, double alpha) {
  if (p == nullptr) return;
  if (i < FPT_SLOTS) {
    p->nlo[i] = alpha;
    p->nhi[i] = alpha;
  } else {
    p->nlo[FPT_SLOTS - 1] = fmin(p->nlo[FPT_SLOTS - 1], alpha);
    p->nhi[FPT_SLOTS - 1] = fmax(p->nhi[FPT_SLOTS - 1], alpha);
  }
}
__device__ __forceinline__ void fpt_finish_slot(FptPred* p, int j, int iters, double alpha_final) {
  if (p == nullptr) return;
  const int K = (iters < FPT_SLOTS) ? iters : FPT_SLOTS;
  if (j >= K) return;
  double l = p->nlo[j], h = p->nhi[j];
  if (j == K - 1) {
    l = fmin(l, alpha_final);
    h = fmax(h, alpha_final);
  }
  double eps = FPT_EPS_NEW, eps_n = FPT_EPS_NEW;
  if (j < p->K && p->K <= FPT_SLOTS) {
    // the drift from call to call is noisy (ADMM iterates oscillate: factors of 5 - 10 between consecutive calls), so the
    // margin follows its recent MAXIMUM: 4 x the last drift, and never below 0.85 of the previous margin.  Replayed on
    // the oracle's iterates of a 32 -> 32 layer (tests/diagnostics/traj_policy_sim.py): 1.3 % of the iterates fall
    // outside their bracket, all of them in the calls right after the start or a change of rho (3 x drift alone: 9 %)
    const double drift = fmax(fabs(l - p->lo[j]), fabs(h - p->hi[j])) / fabs(h);
    eps = fmin(fmax(fmax(4.0 * drift, 0.85 * p->eps[j]), FPT_EPS_MIN), FPT_EPS_MAX);
    // ... while the narrow bracket bets on the next drift being like the last one: most iterates land in it, and its
    // list is a fraction of the wide one's; an iterate that lands between the two costs a scan of the wide list
    eps_n = fmin(fmax(2.5 * drift, FPT_EPS_MIN), eps);
  }
  p->lo[j] = l;
  p->hi[j] = h;
  p->eps[j] = eps;
  p->eps_n[j] = eps_n;
}
// (after every fpt_finish_slot of the call: they read the old K)
__device__ __forceinline__ void fpt_finish_head(FptPred* p, int iters, double sum_abs, int levels) {
  if (p == nullptr) return;
  p->K = (iters < FPT_SLOTS) ? iters : FPT_SLOTS;
  // unit of the next call's integer tallies: (levels - 1) * sum|v| * 2^e < 2^59 leaves a factor 4 for growth
  int e = 0;
  const double bound = (double)(levels - 1) * sum_abs;
  const bool ok = bound > 0.0 && bound < 1e300;
  if (ok) e = 58 - ilogb(bound);
  p->e = e;
  p->e_valid = ok ? 1 : 0;
  p->calls += 1;
}

// Final state of a fixed point that ran on chip (one thread) ...
__device__ __forceinline__ void fp_state_store(effq_fp_state* st, double alpha, double alpha_prev, double sbv,
                                               double sbb, int iters, int done) {
  st->alpha = alpha;
  st->alpha_prev = alpha_prev;
  st->sums[0] = sbv;
  st->sums[1] = sbb;
  st->iters = iters;
  st->done = done;
}
// ... and with the recorder's finish by the same thread (sum_abs: sum |v| of the call)
__device__ __forceinline__ void fp_state_finish(effq_fp_state* st, FptPred* pred, double alpha, double alpha_prev,
                                                double sbv, double sbb, int iters, int done, double sum_abs,
                                                int levels) {
  fp_state_store(st, alpha, alpha_prev, sbv, sbb, iters, done);
  if (pred != nullptr) {
    for (int j = 0; j < FPT_SLOTS; ++j) fpt_finish_slot(pred, j, iters, alpha);
    fpt_finish_head(pred, iters, sum_abs, levels);
  }
}

}  // namespace effq
