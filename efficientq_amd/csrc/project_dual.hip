// The projection + dual update of an ADMM iteration (EfficientQConv.py:108-111, 129-137) as stand-alone kernels: four
// weights per thread where the operands allow 16-byte accesses (proj_vec_ok), else one.  The per-element arithmetic of the
// vector path, and the same projection as the epilogue of a fixed point, are in project_dual.h.
#include "common.h"
#include "fp_level.h"
#include "internal.h"
#include "project_dual.h"

namespace effq {

__global__ __launch_bounds__(TPB) void k_presum(const float* __restrict__ a, const float* __restrict__ b,
                                                float* __restrict__ o, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) o[i] = a[i] + b[i];
}

__global__ __launch_bounds__(TPB) void k_project_dual(const float* __restrict__ v, const float* __restrict__ wstar,
                                                      const effq_fp_state* __restrict__ st, double d,
                                                      float* __restrict__ G, float* __restrict__ dual,
                                                      float dual_div, int8_t* __restrict__ Gq, int lm1, size_t n,
                                                      int32_t* __restrict__ err_flag, ProjNext nx) {
  __builtin_amdgcn_s_setprio(2);   // ADMM chain (critical path) over the loss / inverse streams

  // (optional) the convergence check of the fixed point that produced `st`, folded in to save a launch
  if (err_flag != nullptr && blockIdx.x == 0 && threadIdx.x == 0 && st->done != 1) *err_flag = (st->done == 2) ? 2 : 3;
  const double alpha = st->alpha;
  const float alpha32 = (float)alpha;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double r;
    float b = (float)disc64((double)v[i], alpha, -1.0, 1.0, d, &r);
    float g = alpha32 * b;
    G[i] = g;
    // int8 operand of the exact-integer convs: the signed numerator j' = 2*level - (L-1), or, beyond 128
    // levels where that no longer fits, level - 128 (at 256 levels conv3d_i8s.hip rebuilds j' = 2*(level-128) + 1)
    if (Gq != nullptr) Gq[i] = (lm1 >= 128) ? (int8_t)((int)r - 128) : (int8_t)(2 * (int)r - lm1);
    float du = (wstar[i] - g) + dual[i];        // EfficientQConv.py:111
    if (dual_div != 1.0f) du = du / dual_div;   // "dual /= 2" or "dual /= rho_m/rho" (:131-136)
    dual[i] = du;
    if (nx.Bm != nullptr) {                     // right-hand side of the NEXT prox solve
      const size_t r = i / (size_t)nx.nwrow, k = i - r * (size_t)nx.nwrow;
      nx.Bm[r * (size_t)nx.ldb + k] = prox_rhs(nx.B0[r * (size_t)nx.n + k], nx.W0[i], g, du, nx.eta, nx.rho);
    }
  }
}

// Four consecutive weights per thread (weight rows that are a multiple of 4 long: every layer of the shipped nets): 16-byte
// accesses, one (row, column) split per thread with 32-bit arithmetic, and the level index from the fp32 screen of
// fp_level.h (the reference's fp64 arithmetic decides within 2e-4 of a rounding boundary: indices are exact).
__global__ __launch_bounds__(TPB) void k_project_dual4(const float* __restrict__ v, const float* __restrict__ wstar,
                                                       const effq_fp_state* __restrict__ st, double d,
                                                       float* __restrict__ G, float* __restrict__ dual,
                                                       float dual_div, int8_t* __restrict__ Gq, int lm1, unsigned n4,
                                                       int32_t* __restrict__ err_flag, ProjNext nx) {
  __builtin_amdgcn_s_setprio(2);   // ADMM chain (critical path) over the loss / inverse streams
  if (err_flag != nullptr && blockIdx.x == 0 && threadIdx.x == 0 && st->done != 1) *err_flag = (st->done == 2) ? 2 : 3;
  const double alpha = st->alpha;
  const float alpha32 = (float)alpha;
  const LevelConsts lc = level_consts(alpha, -1.0, 1.0, d);
  const unsigned stride = gridDim.x * blockDim.x;
  for (unsigned q = blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += stride)
    proj4_apply(q, v, wstar, alpha, alpha32, lc, d, G, dual, dual_div, Gq, lm1, nx);
}

}  // namespace effq

using namespace effq;

extern "C" {

int effq_admm_presum(const float* wstar, const float* dual, float* v, size_t n, void* stream) {
  EFFQ_CHECK_ARG(wstar && dual && v);
  if (n == 0) return EFFQ_OK;
  hipLaunchKernelGGL(k_presum, dim3(stream_grid(n)), dim3(TPB), 0, as_stream(stream), wstar, dual, v, n);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// internal (admm_run.hip; internal.h): the one place that checks the arguments and picks the kernel
int effq_project_dual_impl(const float* v, const float* wstar, const effq_fp_state* state_dev, int levels, float* G,
                           float* dual, float dual_div, int8_t* Gq_out, size_t n, int32_t* err_flag_dev,
                           const ProjNext* nx_in, void* stream) {
  EFFQ_CHECK_ARG(v && wstar && state_dev && G && dual && levels >= 2 && levels <= FP_LEVELS_MAX && dual_div > 0.0f);
  ProjNext nx;
  memset(&nx, 0, sizeof(nx));
  if (nx_in != nullptr) {
    nx = *nx_in;
    EFFQ_CHECK_ARG(nx.Bm && nx.B0 && nx.W0 && nx.nwrow > 0 && nx.n >= nx.nwrow && nx.ldb >= nx.n &&
                   (n % (size_t)nx.nwrow) == 0);
  }
  if (n == 0) return EFFQ_OK;
  const double d = 2.0 / (double)(levels - 1);
  if (proj_vec_ok(v, wstar, G, dual, Gq_out, n, nx_in))
    hipLaunchKernelGGL(k_project_dual4, dim3(stream_grid(n / 4)), dim3(TPB), 0, as_stream(stream), v, wstar, state_dev, d,
                       G, dual, dual_div, Gq_out, levels - 1, (unsigned)(n / 4), err_flag_dev, nx);
  else
    hipLaunchKernelGGL(k_project_dual, dim3(stream_grid(n)), dim3(TPB), 0, as_stream(stream), v, wstar, state_dev, d,
                       G, dual, dual_div, Gq_out, levels - 1, n, err_flag_dev, nx);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_admm_project_dual(const float* v, const float* wstar, const effq_fp_state* state_dev, int levels, float* G,
                           float* dual, float dual_div, int8_t* Gq_out, size_t n, void* stream) {
  return effq_project_dual_impl(v, wstar, state_dev, levels, G, dual, dual_div, Gq_out, n, nullptr, nullptr, stream);
}

}  // extern "C"
