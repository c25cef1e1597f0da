// Per-output-channel weight scales: project_by_iter (layer_helper.py:40-70) run on every output row of the weight
// tensor on its own, in ONE launch, with the row's projection + dual update (+ the next prox right-hand side) as the
// epilogue.  The reference has a per-tensor scale only (PTQConv.py:26-27); this is the opt-in channel mode of the
// calibrator (qconv.EfficientQConvHIP, lwq_channel_wise).
//
// Per row c of v = a + b (nwrow values): a0 = mean|v_c|; then b = discretize(v_c / a, L, -1, 1) and
// a <- sum b v_c / sum b b until |a - a_prev| <= tol or max_iter iterations.  A row with sum|v_c| = 0 has no scale (the
// formula divides by zero): it is defined as a = 0, 0 iterations, converged, G_c = 0.
//
// Arithmetic as in k_fp_small (fixed_point_values.hip): the level index from the fp32 screen with the reference's fp64
// arithmetic near a rounding boundary, sum b v = d sum(r v) + lo sum(v), sum b^2 = d^2 sum(r^2) + 2 d lo sum(r) + lo^2 n
// with integer sum(r), sum(r^2); wave sums through the DPP tree with whole waves (absent elements hold 0), waves added in
// wave order: a fixed reduction order, no atomics - two launches give the same bits.
//
// Layout: rows are independent, so there is no grid barrier: one workgroup per row, the row in registers.  Rows of at
// most CH_SHORT values (the first conv: 108, the 1x1x1 classifier: 32, the 32-channel 3^3 layers: 864) take one wave
// and no LDS barrier at all; longer rows (up to 16384: the 512-channel 3^3 layers of LiTS have 13824) take 256 threads
// and one LDS barrier per iteration.
#include "common.h"
#include "project_dual.h"

namespace effq {

constexpr int CH_SHORT = 1024;           // rows up to this length: one wave per row (T = 64, PER <= 16)
constexpr int CH_MAX_ROW = 256 * 64;     // T = 256, PER <= 64

struct ChanOut {
  double* alpha;          // [c2]
  int32_t* iters;         // [c2] or nullptr
  int32_t* err_flag;      // sticky 2 when a row hit max_iter, or nullptr
};

template <int T, int PER>
__global__ __launch_bounds__(T) void k_fp_channels(const float* __restrict__ a, const float* b2, float* v_out, int nwrow,
                                                   double lo, double hi, double d, double tol, int max_iter, ChanOut out,
                                                   ProjFused pf) {
  constexpr int NW = T / 64;
  __shared__ double part[2][3][NW];
  __builtin_amdgcn_s_setprio(3);           // on the critical path of the ADMM chain, as k_fp_small
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int row = blockIdx.x;
  const size_t base = (size_t)row * (size_t)nwrow;
  float vr[PER];
  double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int c = tid + k * T;
    float v = 0.0f;                        // absent elements: v = 0, lanes stay active (the DPP tree needs whole waves)
    if (c < nwrow) {
      v = (b2 != nullptr) ? (a[base + c] + b2[base + c]) : a[base + c];
      if (v_out != nullptr) v_out[base + c] = v;
    }
    vr[k] = v;
    acc0 += fabs((double)v);
    acc1 += (double)v;
  }
  acc0 = wave_sum_f64_dpp(acc0);
  acc1 = wave_sum_f64_dpp(acc1);
  double tot = acc0, sv = acc1;            // sum |v|, sum v
  if (NW > 1) {
    if (lane == 0) {
      part[0][0][wid] = acc0;
      part[0][1][wid] = acc1;
    }
    lds_barrier();
    tot = 0.0;
    sv = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      tot += part[0][0][w];
      sv += part[0][1][w];
    }
  }
  const double n = (double)nwrow;
  const bool zero_row = !(tot != 0.0);
  double alpha = zero_row ? 0.0 : tot / n;
  double ralpha = zero_row ? 0.0 : n / tot;
  int it = 0, done = zero_row ? 1 : 0;
  const double rd = 1.0 / d;
  LevelConsts lc = level_grid(lo, hi, d);
  while (!done) {
    const int par = (it + 1) & 1;          // parity 0 carried the prologue sums
    lc.c1 = (float)(ralpha * rd);
    double arv = 0.0;
    int sr = 0, sr2 = 0;                   // <= 64 slots x 255^2 per thread
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const float vf = vr[k];
      const float rf = fp_level_f(vf, lc, alpha, lo, hi, d);
      const int ri = (tid + k * T < nwrow) ? (int)rf : 0;     // absent elements must not count
      sr += ri;
      sr2 += ri * ri;
      arv = __builtin_fma((double)rf, (double)vf, arv);       // r v exact in fp64; absent elements have v = 0
    }
    arv = wave_sum_f64_dpp(arv);
    const unsigned wr = group_sum_u32((unsigned)sr, 64), wr2 = group_sum_u32((unsigned)sr2, 64);
    double trv = arv, tr = (double)wr, tr2 = (double)wr2;
    if (NW > 1) {
      if (lane == 0) {
        part[par][0][wid] = arv;
        part[par][1][wid] = (double)wr;
        part[par][2][wid] = (double)wr2;
      }
      lds_barrier();
      trv = 0.0;
      tr = 0.0;
      tr2 = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        trv += part[par][0][w];
        tr += part[par][1][w];
        tr2 += part[par][2][w];
      }
    }
    const double t0 = level_sum_bv(trv, sv, lo, d);   // sum b v
    const double t1 = level_sum_bb(tr2, tr, n, lo, d);   // sum b^2
    const double a_new = t0 / t1;
    const double ra_new = t1 / t0;
    ++it;
    fp_stop(it, max_iter, a_new, alpha, tol, done);
    alpha = a_new;
    ralpha = ra_new;
  }
  if (tid == 0) {
    out.alpha[row] = alpha;
    if (out.iters != nullptr) out.iters[row] = it;
    if (out.err_flag != nullptr && done == 2) *out.err_flag = 2;
  }
  if (pf.G != nullptr) {                   // this row's projection + dual update (+ Bm of the next prox solve)
    const float alpha32 = (float)alpha;
    const LevelConsts plc = level_consts(zero_row ? 1.0 : alpha, -1.0, 1.0, pf.d);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int c = tid + k * T;
      if (c < nwrow)
        proj1_apply(base + c, (unsigned)row, (unsigned)c, vr[k], alpha, alpha32, plc, pf.d, zero_row, pf.wstar, pf.G,
                    pf.dual, pf.dual_div, pf.nx);
    }
  }
}

static int fp_channels_launch(const float* a, const float* b, float* v_out, int c2, int nwrow, int levels, double tol,
                              int max_iter, double* alpha_out, int32_t* iters_out, int32_t* err_flag,
                              const ProjFused& pf, hipStream_t st) {
  const double lo = -1.0, hi = 1.0, d = (hi - lo) / (double)(levels - 1);
  ChanOut o;
  o.alpha = alpha_out;
  o.iters = iters_out;
  o.err_flag = err_flag;
  const dim3 grid((unsigned)c2);
#define FPCH(TT, PP) \
  hipLaunchKernelGGL((k_fp_channels<TT, PP>), grid, dim3(TT), 0, st, a, b, v_out, nwrow, lo, hi, d, tol, max_iter, o, pf)
  if (nwrow <= 64) FPCH(64, 1);
  else if (nwrow <= 128) FPCH(64, 2);
  else if (nwrow <= 256) FPCH(64, 4);
  else if (nwrow <= 512) FPCH(64, 8);
  else if (nwrow <= CH_SHORT) FPCH(64, 16);
  else if (nwrow <= 2048) FPCH(256, 8);
  else if (nwrow <= 4096) FPCH(256, 16);
  else if (nwrow <= 8192) FPCH(256, 32);
  else FPCH(256, 64);
#undef FPCH
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_fp_channels_max_row(void) { return CH_MAX_ROW; }

int effq_fixed_point_channels(const float* a, const float* b, float* v_out, int c2, int nwrow, int levels, double tol,
                              int max_iter, double* alpha_out, int32_t* iters_out, int32_t* err_flag_dev, void* stream) {
  EFFQ_CHECK_ARG(a && alpha_out && c2 > 0 && nwrow > 0 && nwrow <= CH_MAX_ROW && levels >= 2 && levels <= 256 &&
                 max_iter > 0);
  EFFQ_CHECK_ARG(b == nullptr || v_out != nullptr);
  ProjFused pf;
  memset(&pf, 0, sizeof(pf));
  return fp_channels_launch(a, b, v_out, c2, nwrow, levels, tol, max_iter, alpha_out, iters_out, err_flag_dev, pf,
                            as_stream(stream));
}

int effq_fixed_point_channels_proj(const float* wstar, float* dual, float* v_out, int c2, int nwrow, int levels,
                                   double tol, int max_iter, double* alpha_out, int32_t* iters_out, int32_t* err_flag_dev,
                                   float* G, float dual_div, float* Bm, const float* B0, const float* W0, int n, int ldb,
                                   double rho_next, double eta, void* stream) {
  EFFQ_CHECK_ARG(wstar && dual && v_out && G && alpha_out && c2 > 0 && nwrow > 0 && nwrow <= CH_MAX_ROW && levels >= 2 &&
                 levels <= 256 && max_iter > 0 && dual_div > 0.0f);
  EFFQ_CHECK_ARG(Bm == nullptr || (B0 && W0 && n >= nwrow && ldb >= nwrow));
  ProjFused pf;
  memset(&pf, 0, sizeof(pf));
  pf.wstar = wstar;
  pf.G = G;
  pf.dual = dual;
  pf.d = 2.0 / (double)(levels - 1);
  pf.dual_div = dual_div;
  pf.lm1 = levels - 1;
  if (Bm != nullptr) {
    pf.nx.Bm = Bm; pf.nx.B0 = B0; pf.nx.W0 = W0; pf.nx.nwrow = nwrow; pf.nx.n = n; pf.nx.ldb = ldb;
    pf.nx.rho = (float)rho_next; pf.nx.eta = (float)eta;
  }
  return fp_channels_launch(wstar, dual, v_out, c2, nwrow, levels, tol, max_iter, alpha_out, iters_out, err_flag_dev, pf,
                            as_stream(stream));
}

}  // extern "C"
