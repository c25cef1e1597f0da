// The library's error string, the scalar quantisers, the fp64 reductions with the per-iteration fixed point built on them
// (k_fp_iter: one launch per iteration), the training helpers and the bit packing: HBM-bound streaming kernels.  (The
// single-launch weight fixed points are in fixed_point_values.hip, the ADMM projection in project_dual.hip.)
// Reference: layer_helper.py:25-70 (discretize, project_by_iter), PTQConv.py:114-116.
// All arithmetic follows the reference's operation order with IEEE divisions and no FMA
// contraction (the library is built with -ffp-contract=off).
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include "common.h"
#include "fp_level.h"
#include "internal.h"

namespace effq {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- scalar quantiser bodies ----------------------------------------------------------
__device__ __forceinline__ float qd32(float x, float alpha, float lo, float hi, float d, float* idx) {
  float t = x / alpha;
  t = fminf(fmaxf(t, lo), hi);
  // torch.clamp propagates NaN; fmaxf/fminf would drop it
  t = (x != x) ? x : t;
  float r = rintf((t - lo) / d);
  *idx = r;
  return (r * d + lo) * alpha;
}

// Same level index as disc64 (bit-exact), without the two IEEE fp64 divisions on the common path: the
// quotient is formed with reciprocals (a few ulp off) and accepted only when it is provably on the same
// side of every rounding boundary as the exact one; otherwise the exact divisions are redone.
__device__ __forceinline__ double disc64_fast(double x, double alpha, double ralpha, double lo, double hi, double d,
                                              double rd, double* idx) {
  double t = fmin(fmax(x * ralpha, lo), hi);
  const double u = (t - lo) * rd;
  const double fr = u - floor(u);
  // |u_exact - u| <= ~8 ulp(u) + the clamp edges; 1e-9 is far above that and far below any real margin
  // (a few-ulp change of t at a clamp edge moves u by a few ulp next to an INTEGER, which rint absorbs)
  const bool safe = fabs(fr - 0.5) > 1e-9 * (1.0 + u);
  if (safe) {
    const double r = rint(u);
    *idx = r;
    return r * d + lo;
  }
  return disc64(x, alpha, lo, hi, d, idx);
}

// Statistics of one fixed-point pass without per-value fp64 arithmetic beyond one multiply-add: the level index r from the
// fp32 screen (fp_level.h), exactly the reference's, and integer tallies from which level_sum_bv / _bb form sum b x, sum b^2.
// four doubles of scratch in the tail of the reduction workspace (after the ticket and the cooperative kernel's two
// counter words at +64 / +68): the raw totals of a level-statistics pass before level_finish
__device__ __forceinline__ double* level_scratch(double* partials) {
  return reinterpret_cast<double*>(reinterpret_cast<char*>(partials) + sizeof(double) * RED_MAX_BLOCKS * RED_SLOTS + 128);
}
struct LevelStats {
  double arx, sx;          // sum r x, sum x (sx only when lo != 0)
  long long sr, sr2;       // sum r, sum r^2
};
struct LevelPass {         // the scale and the level grid of a pass
  LevelConsts c;
  double alpha, lo, hi, d;
  bool need_sx;
};
__device__ __forceinline__ LevelPass level_pass(double alpha, double lo, double hi, double d) {
  return {level_consts(alpha, lo, hi, d), alpha, lo, hi, d, lo != 0.0};
}
__device__ __forceinline__ void level_accum(float xf, const LevelPass& p, LevelStats& a) {
  const float rf = fp_level_f(xf, p.c, p.alpha, p.lo, p.hi, p.d);
  const int ri = (int)rf;
  a.sr += ri;
  a.sr2 += ri * ri;
  a.arx = __builtin_fma((double)rf, (double)xf, a.arx);
  if (p.need_sx) a.sx += (double)xf;
}
// [sum r x, sum r, sum r^2, sum x] over n values -> [sum b x, sum b b]
__device__ __forceinline__ void level_finish(const double* t4, size_t n, double lo, double d, double* out2) {
  out2[0] = level_sum_bv(t4[0], t4[3], lo, d);
  out2[1] = level_sum_bb(t4[2], t4[1], n, lo, d);
}

__global__ __launch_bounds__(TPB) void k_quant_dequant_f32(const float* __restrict__ x,
                                                           const float* __restrict__ alpha_dev, float lo,
                                                           float hi, float d, float* __restrict__ y,
                                                           uint8_t* __restrict__ idx, size_t n) {
  const float alpha = *alpha_dev;
  const size_t nv = n / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    float r0, r1, r2, r3;
    float4 o;
    o.x = qd32(v.x, alpha, lo, hi, d, &r0);
    o.y = qd32(v.y, alpha, lo, hi, d, &r1);
    o.z = qd32(v.z, alpha, lo, hi, d, &r2);
    o.w = qd32(v.w, alpha, lo, hi, d, &r3);
    if (y) reinterpret_cast<float4*>(y)[i] = o;
    if (idx) {
      uchar4 u = make_uchar4((unsigned char)r0, (unsigned char)r1, (unsigned char)r2, (unsigned char)r3);
      reinterpret_cast<uchar4*>(idx)[i] = u;
    }
  }
  // ragged tail
  for (size_t i = nv * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float r;
    float o = qd32(x[i], alpha, lo, hi, d, &r);
    if (y) y[i] = o;
    if (idx) idx[i] = (unsigned char)r;
  }
}

// b of the fp64 path: disc64 rounded to fp32, with torch.clamp's NaN propagation as in qd32 (the fmin / fmax of
// level_exact drop a NaN and would return lo for it); the level id of a NaN is unspecified (include/effq_hip.h)
__device__ __forceinline__ float qd64(float x, double alpha, double lo, double hi, double d, double* idx) {
  const float b = (float)disc64((double)x, alpha, lo, hi, d, idx);
  return (x != x) ? x : b;
}

__global__ __launch_bounds__(TPB) void k_quant_dequant_f64path(const float* __restrict__ x,
                                                               const double* __restrict__ alpha_dev, double lo,
                                                               double hi, double d, float* __restrict__ y,
                                                               float* __restrict__ bout,
                                                               uint8_t* __restrict__ idx, size_t n) {
  const double alpha = *alpha_dev;
  const float alpha32 = (float)alpha;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nv = n / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    double r0, r1, r2, r3;
    float4 b;
    b.x = qd64(v.x, alpha, lo, hi, d, &r0);
    b.y = qd64(v.y, alpha, lo, hi, d, &r1);
    b.z = qd64(v.z, alpha, lo, hi, d, &r2);
    b.w = qd64(v.w, alpha, lo, hi, d, &r3);
    if (bout) reinterpret_cast<float4*>(bout)[i] = b;
    if (y) {
      float4 o = make_float4(alpha32 * b.x, alpha32 * b.y, alpha32 * b.z, alpha32 * b.w);
      reinterpret_cast<float4*>(y)[i] = o;
    }
    if (idx)
      reinterpret_cast<uchar4*>(idx)[i] =
          make_uchar4((unsigned char)r0, (unsigned char)r1, (unsigned char)r2, (unsigned char)r3);
  }
  for (size_t i = nv * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double r;
    float b = qd64(x[i], alpha, lo, hi, d, &r);
    if (bout) bout[i] = b;
    if (y) y[i] = alpha32 * b;
    if (idx) idx[i] = (unsigned char)r;
  }
}

// ---- fp64 reductions ---------------------------------------------------------------------
// MODE 0: sum|x|, n     MODE 1: sum x, sum x^2, n     MODE 2: sum b*x, sum b*b  (b=discretize(x/alpha))
template <int MODE>
__global__ __launch_bounds__(TPB) void k_reduce(const float* __restrict__ x, size_t n,
                                                const double* __restrict__ alpha_dev, double lo, double hi,
                                                double d, const int32_t* __restrict__ done_flag,
                                                double* partials, unsigned int* ticket, double* out) {
  constexpr int NS = (MODE == 1) ? 3 : (MODE == 2) ? 4 : 2;
  __shared__ double smem[NS * 16];
  __shared__ int s_last;
  if (MODE == 2 && done_flag != nullptr && *done_flag != 0) return;  // uniform across the grid
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;
  LevelStats ls = {0.0, 0.0, 0, 0};
  const LevelPass lp = level_pass((MODE == 2) ? *alpha_dev : 1.0, lo, hi, (MODE == 2) ? d : 1.0);
  const size_t nv = n / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  auto body = [&](float xf) {
    if (MODE == 0) {
      acc[0] += fabs((double)xf);
    } else if (MODE == 1) {
      const double v = (double)xf;
      acc[0] += v;
      acc[1] += v * v;
    } else {
      level_accum(xf, lp, ls);
    }
  };
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    body(v.x);
    body(v.y);
    body(v.z);
    body(v.w);
  }
  for (size_t i = nv * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) body(x[i]);
  if (MODE != 2) {
    if (blockIdx.x == 0 && threadIdx.x == 0) acc[NS - 1] = (double)n;
    grid_sum_finish<NS>(acc, partials, ticket, out, smem, &s_last);
  } else {
    acc[0] = ls.arx; acc[1] = (double)ls.sr; acc[2] = (double)ls.sr2; acc[NS - 1] = ls.sx;
    double* t4 = level_scratch(partials);
    grid_sum_finish<NS>(acc, partials, ticket, t4, smem, &s_last);
    if (s_last && threadIdx.x == 0) level_finish(t4, n, lo, d, out);
  }
}


// ---- fused fixed-point iteration: statistics pass whose last-arriving block also performs the scalar
// update (layer_helper.py:55-60), so one launch = one iteration.  Used where no all-reduce sits between
// the two (replicated weights; single-GPU activations).
__global__ __launch_bounds__(TPB) void k_fp_iter(const float* __restrict__ x, size_t n, effq_fp_state* st, double lo,
                                                 double hi, double d, double tol, int max_iter, double* partials,
                                                 unsigned int* ticket) {
  __shared__ double smem[4 * 16];
  __shared__ int s_last;
  if (st->done != 0) return;  // uniform across the grid
  const double alpha = st->alpha;
  const LevelPass lp = level_pass(alpha, lo, hi, d);
  LevelStats ls = {0.0, 0.0, 0, 0};
  const size_t nv = n / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    level_accum(v.x, lp, ls);
    level_accum(v.y, lp, ls);
    level_accum(v.z, lp, ls);
    level_accum(v.w, lp, ls);
  }
  for (size_t i = nv * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    level_accum(x[i], lp, ls);
  double acc[4] = {ls.arx, (double)ls.sr, (double)ls.sr2, ls.sx};
  double* t4 = level_scratch(partials);
  grid_sum_finish<4>(acc, partials, ticket, t4, smem, &s_last);
  if (s_last && threadIdx.x == 0) level_finish(t4, n, lo, d, st->sums);
  // the finishing block has written the sums into st->sums; it then applies the update
  if (s_last && threadIdx.x == 0) {
    const double a_new = st->sums[0] / st->sums[1];
    st->alpha_prev = alpha;
    st->alpha = a_new;
    const int it = st->iters + 1;
    st->iters = it;
    fp_stop(it, max_iter, a_new, alpha, tol, st->done);
  }
}

__global__ void k_fp_init(effq_fp_state* st, const double* abs_sums) {
  st->alpha = abs_sums[0] / abs_sums[1];
  st->alpha_prev = -999.0;
  st->sums[0] = 0.0;
  st->sums[1] = 0.0;
  st->iters = 0;
  st->done = 0;
}

__global__ void k_fp_update(effq_fp_state* st, double tol, int max_iter) {
  if (st->done) return;
  // loop head of layer_helper.py:55: while abs(a - a_prev) > 1e-5 and c < max_iter
  double a_new = st->sums[0] / st->sums[1];
  st->alpha_prev = st->alpha;
  st->alpha = a_new;
  st->iters += 1;
  fp_stop(st->iters, max_iter, st->alpha, st->alpha_prev, tol, st->done);
}

// ---- backward of PTQConv._quantize_act with the straight-through estimator (row f3) ------------------------------------
// q = discretize(x / alpha, L, 0, 1) * alpha (PTQConv.py:114-116), round with identity gradient (layer_helper.py:13-22),
// clamp with torch's gradient mask (1 where lo <= u <= hi, bounds included).  With u = x / alpha, r = discretize(u):
//   dq/dx = mask,    dq/dalpha = r - mask * u          =>   gx = gq * mask,   galpha = sum gq * (r - mask * u)
// (the chain rule autograd applies to the reference's five elementwise ops, collected into one pass).
__global__ __launch_bounds__(TPB) void k_act_quant_bwd(const float* __restrict__ x, const float* __restrict__ alpha_dev,
                                                       float lo, float hi, float d, const float* __restrict__ gq,
                                                       float* __restrict__ gx, size_t n, double* partials,
                                                       unsigned int* ticket, double* galpha_out) {
  __shared__ double smem[16];
  __shared__ int s_last;
  const float alpha = *alpha_dev;
  double acc[1] = {0.0};
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float u = x[i] / alpha;
    const float c = fminf(fmaxf(u, lo), hi);
    const float r = rintf((c - lo) / d) * d + lo;
    const float m = (u >= lo && u <= hi) ? 1.0f : 0.0f;
    const float g = gq[i];
    if (gx != nullptr) gx[i] = g * m;
    acc[0] += (double)(g * (r - m * u));
  }
  grid_sum_finish<1>(acc, partials, ticket, galpha_out, smem, &s_last);
}

__global__ __launch_bounds__(TPB) void k_adam(float* __restrict__ p, const float* __restrict__ g,
                                              float* __restrict__ m, float* __restrict__ v, float w1, float b2,
                                              float w2, float eps, float step, float bc2_sqrt, size_t n) {
  // torch.optim.Adam (no weight decay, no amsgrad): ptqer.py:255 Adam(opt_param, lr=5e-4).  w1 = 1 - beta1, w2 = 1 - beta2,
  // step = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t): formed in double on the host and rounded once, as torch does
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float gi = g[i];
    float mi = m[i] + w1 * (gi - m[i]);                   // lerp form used by torch
    float vi = b2 * v[i] + w2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = p[i] - step * (mi / denom);
  }
}

// ---- bit-packed storage of level ids (row f2: the reference stores one uint8 per weight, PTQConv.py:125-152) ----
// element i occupies bits [i*bits, (i+1)*bits) of the little-endian bit stream; bits in {1, 2, 4, 8}
__global__ __launch_bounds__(TPB) void k_pack_levels(const uint8_t* __restrict__ idx, size_t n, int bits,
                                                     uint8_t* __restrict__ packed, size_t nbytes) {
  const int per = 8 / bits;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < nbytes; b += stride) {
    unsigned v = 0;
    for (int k = 0; k < per; ++k) {
      const size_t i = b * per + k;
      if (i < n) v |= ((unsigned)idx[i] & ((1u << bits) - 1u)) << (k * bits);
    }
    packed[b] = (uint8_t)v;
  }
}

__global__ __launch_bounds__(TPB) void k_unpack_levels(const uint8_t* __restrict__ packed, size_t n, int bits,
                                                       uint8_t* __restrict__ idx) {
  const int per = 8 / bits;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    idx[i] = (uint8_t)((packed[i / per] >> ((i % per) * bits)) & ((1u << bits) - 1u));
}

}  // namespace effq

using namespace effq;

extern "C" {

const char* effq_last_error(void) { return g_err; }
int effq_version(void) { return 100; }

int effq_device_count(int* count) {
  EFFQ_CHECK_ARG(count != nullptr);
  EFFQ_HIP(hipGetDeviceCount(count));
  return EFFQ_OK;
}

size_t effq_reduce_ws_bytes(void) { return RED_WS_BYTES; }

int effq_quant_dequant_f32(const float* x, const float* alpha_dev, float lo, float hi, int levels, float* y_out,
                           uint8_t* idx_out, size_t n, void* stream) {
  if (n == 0) return EFFQ_OK;  /* empty tensors are legal (and carry null pointers) */
  EFFQ_CHECK_ARG(x && alpha_dev && levels >= 2 && hi > lo);
  EFFQ_CHECK_ARG(idx_out == nullptr || levels <= 256);
  const float d = (float)(((double)hi - (double)lo) / (double)(levels - 1));
  hipLaunchKernelGGL(k_quant_dequant_f32, dim3(stream_grid((n + 3) / 4)), dim3(TPB), 0, as_stream(stream), x,
                     alpha_dev, lo, hi, d, y_out, idx_out, n);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_quant_dequant_f64path(const float* x, const double* alpha_dev, double lo, double hi, int levels,
                               float* y_out, float* b_out, uint8_t* idx_out, size_t n, void* stream) {
  if (n == 0) return EFFQ_OK;  /* empty tensors are legal (and carry null pointers) */
  EFFQ_CHECK_ARG(x && alpha_dev && levels >= 2 && hi > lo);
  EFFQ_CHECK_ARG(idx_out == nullptr || levels <= 256);
  const double d = (hi - lo) / (double)(levels - 1);
  hipLaunchKernelGGL(k_quant_dequant_f64path, dim3(stream_grid((n + 3) / 4)), dim3(TPB), 0, as_stream(stream), x,
                     alpha_dev, lo, hi, d, y_out, b_out, idx_out, n);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_abs_sum_f64(const float* x, size_t n, double* sums_out, void* ws, void* stream) {
  EFFQ_CHECK_ARG(x && sums_out && ws && n > 0);
  RedWs r = red_ws(ws);
  hipLaunchKernelGGL(k_reduce<0>, dim3(stream_grid((n + 3) / 4)), dim3(TPB), 0, as_stream(stream), x, n,
                     (const double*)nullptr, 0.0, 0.0, 0.0, (const int32_t*)nullptr, r.partials, r.ticket,
                     sums_out);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_moments_f64(const float* x, size_t n, double* sums_out, void* ws, void* stream) {
  EFFQ_CHECK_ARG(x && sums_out && ws && n > 0);
  RedWs r = red_ws(ws);
  hipLaunchKernelGGL(k_reduce<1>, dim3(stream_grid((n + 3) / 4)), dim3(TPB), 0, as_stream(stream), x, n,
                     (const double*)nullptr, 0.0, 0.0, 0.0, (const int32_t*)nullptr, r.partials, r.ticket,
                     sums_out);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_alpha_stats_f64(const float* x, const double* alpha_dev, double lo, double hi, int levels, size_t n,
                         double* sums_out, const int32_t* done_flag_dev, void* ws, void* stream) {
  EFFQ_CHECK_ARG(x && alpha_dev && sums_out && ws && n > 0 && levels >= 2 && levels <= FP_LEVELS_MAX && hi > lo);
  RedWs r = red_ws(ws);
  const double d = (hi - lo) / (double)(levels - 1);
  hipLaunchKernelGGL(k_reduce<2>, dim3(stream_grid((n + 3) / 4)), dim3(TPB), 0, as_stream(stream), x, n, alpha_dev,
                     lo, hi, d, done_flag_dev, r.partials, r.ticket, sums_out);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_fp_init(effq_fp_state* state_dev, const double* abs_sums_dev, void* stream) {
  EFFQ_CHECK_ARG(state_dev && abs_sums_dev);
  hipLaunchKernelGGL(k_fp_init, dim3(1), dim3(1), 0, as_stream(stream), state_dev, abs_sums_dev);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_fp_update(effq_fp_state* state_dev, double tol, int max_iter, void* stream) {
  EFFQ_CHECK_ARG(state_dev && max_iter > 0);
  hipLaunchKernelGGL(k_fp_update, dim3(1), dim3(1), 0, as_stream(stream), state_dev, tol, max_iter);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_alpha_fixed_point(const float* x, size_t n, int levels, double lo, double hi, double tol, int max_iter,
                           int n_iters, effq_fp_state* state_dev, void* ws, void* stream) {
  EFFQ_CHECK_ARG(x && state_dev && ws && n > 0 && n_iters >= 0 && levels >= 2 && levels <= FP_LEVELS_MAX && hi > lo);
  RedWs r = red_ws(ws);
  const double d = (hi - lo) / (double)(levels - 1);
  const int grid = stream_grid((n + 3) / 4);
  for (int i = 0; i < n_iters; ++i)
    hipLaunchKernelGGL(k_fp_iter, dim3(grid), dim3(TPB), 0, as_stream(stream), x, n, state_dev, lo, hi, d, tol,
                       max_iter, r.partials, r.ticket);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_act_quant_backward(const float* x, const float* alpha_dev, int levels, const float* gq, float* gx_out,
                            double* galpha_out, size_t n, void* ws, void* stream) {
  EFFQ_CHECK_ARG(x && alpha_dev && gq && galpha_out && ws && n > 0 && levels >= 2);
  RedWs r = red_ws(ws);
  const float d = (float)(1.0 / (double)(levels - 1));
  hipLaunchKernelGGL(k_act_quant_bwd, dim3(stream_grid(n)), dim3(TPB), 0, as_stream(stream), x, alpha_dev, 0.0f, 1.0f, d,
                     gq, gx_out, n, r.partials, r.ticket, galpha_out);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_adam_step(float* p, const float* g, float* m, float* v, double lr, double b1, double b2, double eps, int t,
                   size_t n, void* stream) {
  EFFQ_CHECK_ARG(t >= 1);
  if (n == 0) return EFFQ_OK;  /* an empty parameter vector is legal (and carries null pointers) */
  EFFQ_CHECK_ARG(p && g && m && v);
  // 1 - (float)0.999 is 1.3e-5 off 1 - 0.999, and that error does not cancel against 1 - beta2^t once t is large
  const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
  hipLaunchKernelGGL(k_adam, dim3(stream_grid(n)), dim3(TPB), 0, as_stream(stream), p, g, m, v, (float)(1.0 - b1),
                     (float)b2, (float)(1.0 - b2), (float)eps, (float)(lr / bc1), (float)sqrt(bc2), n);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

size_t effq_packed_bytes(size_t n, int bits) {
  if (!(bits == 1 || bits == 2 || bits == 4 || bits == 8)) return 0;
  return (n * (size_t)bits + 7) / 8;
}

int effq_pack_levels(const uint8_t* idx, size_t n, int bits, uint8_t* packed, void* stream) {
  EFFQ_CHECK_ARG(bits == 1 || bits == 2 || bits == 4 || bits == 8);
  if (n == 0) return EFFQ_OK;
  EFFQ_CHECK_ARG(idx && packed);
  const size_t nbytes = effq_packed_bytes(n, bits);
  hipLaunchKernelGGL(k_pack_levels, dim3(stream_grid(nbytes)), dim3(TPB), 0, as_stream(stream), idx, n, bits, packed,
                     nbytes);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_unpack_levels(const uint8_t* packed, size_t n, int bits, uint8_t* idx, void* stream) {
  EFFQ_CHECK_ARG(bits == 1 || bits == 2 || bits == 4 || bits == 8);
  if (n == 0) return EFFQ_OK;
  EFFQ_CHECK_ARG(idx && packed);
  hipLaunchKernelGGL(k_unpack_levels, dim3(stream_grid(n)), dim3(TPB), 0, as_stream(stream), packed, n, bits, idx);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
