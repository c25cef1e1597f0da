// The kernels of --prep_bias n4 (bias.py, where the rule stands; restated in include/effq_hip.h):
//   effq_prep_bias_log    u = log(v) and the fit mask M of one scan;
//   effq_prep_bias_hist   min, max and count of r = u - f over the samples in M, then the 200 fixed-point counters;
//   effq_prep_bias_fit    e = r - lerp(E, r), the least-squares lattice phi of e at one level, Phi += phi, f += eval(phi)
//                         on the samples, and the two sums of the convergence measure;
//   effq_prep_bias_apply  v / exp(f) on the full grid from the four lattices.
//
// Samples.  Every kernel takes the sample stride s and offset o per axis: sample q of an axis is the full-grid index
// x = s q + o, and the spline coordinate is always that of the full grid, t = (x + 0.5) / X * n (bias_weights).  f lives
// on the samples only, a dense OD x OH x OW fp32 array.
//
// The fit.  The 64 weights of a sample are a tensor product and so is S, the sum of their squares, so
//   delta[a][b][c] = sum_d A3d[d][a] sum_h A3h[h][b] sum_w A3w[w][c] e m,      A3 = w^3 / (the axis' sum of w^2),
//   omega[a][b][c] = the same with A2 = w^2 and m for e m,
// three contractions with banded matrices of at most 11 columns.  k_bias_fit_partial: a workgroup owns a slab, 32 rows of
// one sampled plane.  It walks W in chunks of 64 samples: the chunk's two banded matrices go to LDS as dense 64 x 16 fp64
// (thread (x, quarter) forms the weights of x and writes four columns, zeros outside the band), e m and m of 32 x 64
// samples go to LDS as fp32 (the row pitch 65 keeps the 32 rows of a wave on 32 banks), and thread (row, column group)
// multiplies its row with columns cg and cg + 8 of both matrices: a 32 x 64 x 16 product in plain fp64 FMAs, no predicate
// in the loop.  The H contraction runs inside the workgroup on the 32 x 16 results, and the slab leaves one fp64 partial
// of 2 x P x P.  k_bias_fit_lattice: one wave per control point, lane i adds the partials i, i + 64, ... of the planes
// of its band in order, a fixed butterfly adds the lanes, lane 0 divides, writes phi and adds it to Phi (one thread per
// point took 532 us of a 780 us call at stride 1: DESIGN section 30).  k_bias_fit_eval: a wave owns a sample row, its first P lanes
// contract phi with the plane's and the row's weights into P row coefficients, and every lane picks its four by
// __shfl; f += fp32(df), and exp(df) and its square are summed over M by the fixed tree of common.h (grid_sum_finish).
// No floating-point atomic anywhere: equal inputs give equal bits.  No workgroup waits for another.
//
// The W contraction is 32 fp64 FMAs per sample (two matrices of 16 columns) in plain FMAs.  The fp64 matrix instruction
// was not tried and not timed: in the kernel trace of DESIGN section 30 k_bias_fit_partial is the smaller part of a fit
// call, so the instruction could win little there; the fp32 ones would round the sums the tests' bound rests on.
#include <math.h>
#include "common.h"
#include "prep_rows.h"

namespace effq {

constexpr int BIAS_BINS = EFFQ_PREP_BIAS_BINS;
constexpr int BIAS_LEVELS = EFFQ_PREP_BIAS_LEVELS;
constexpr int BIAS_MAX_P = (1 << (BIAS_LEVELS - 1)) + 3;      // 11 control points per axis at the finest level
constexpr int BIAS_LATTICE = EFFQ_PREP_BIAS_LATTICE;          // 4^3 + 5^3 + 7^3 + 11^3 doubles, level after level
constexpr int BIAS_COLS = 16, BIAS_ROWS = 32, BIAS_WC = 64;
constexpr int BIAS_FRAC = 65536;
static_assert(BIAS_MAX_P <= BIAS_COLS && BIAS_LATTICE == 64 + 125 + 343 + 1331 && BIAS_ROWS * 8 == PREP_THREADS,
              "the shape of the fit");

struct BiasGrid {
  unsigned D, H, W;          // the full grid
  unsigned s[3], o[3];       // the sample stride and offset per axis
  unsigned OD, OH, OW;       // the samples per axis
};

struct BiasW {
  int k;
  double w[4];
};
// Span and the four uniform cubic B-spline weights of full-grid index x of an axis of length X at n spans.
__device__ __forceinline__ BiasW bias_weights(unsigned x, unsigned X, int n) {
  BiasW r;
  const double t = ((double)x + 0.5) / (double)X * (double)n;
  r.k = (int)t;
  if (r.k > n - 1) r.k = n - 1;
  const double a = t - (double)r.k, a2 = a * a, a3 = a2 * a, b = 1.0 - a;
  r.w[0] = b * b * b / 6.0;
  r.w[1] = (3.0 * a3 - 6.0 * a2 + 4.0) / 6.0;
  r.w[2] = (-3.0 * a3 + 3.0 * a2 + 3.0 * a + 1.0) / 6.0;
  r.w[3] = a3 / 6.0;
  return r;
}
__device__ __forceinline__ double pick4(const double (&w)[4], int j) {      // w[j], 0 outside 0 .. 3; no indexed register
  double v = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) v = (j == i) ? w[i] : v;
  return v;
}
__device__ __forceinline__ double sum_sq4(const double (&w)[4]) { return w[0] * w[0] + w[1] * w[1] + w[2] * w[2] + w[3] * w[3]; }

// The position of r between the bin centres lo + i (hi - lo) / 199, all fp64: t = (r - lo) * inv, inv = 199 / (hi - lo).
__device__ __forceinline__ void bias_bin(float r, float lo, double inv, int& k, double& frac) {
  const double t = ((double)r - (double)lo) * inv;
  k = t > 0.0 ? (int)t : 0;
  if (k > BIAS_BINS - 2) k = BIAS_BINS - 2;
  frac = t - (double)k;
  frac = frac < 0.0 ? 0.0 : (frac > 1.0 ? 1.0 : frac);
}

// An order-preserving map of finite floats to uint32, so that min and max are integer atomics.
__device__ __forceinline__ unsigned enc_float(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec_float(unsigned e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}
__device__ __forceinline__ void wave_min_max(float& lo, float& hi) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, 64));
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
  }
}

// ---- log -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PREP_THREADS) void k_bias_log(const float* v, float* u, uint8_t* m, unsigned total,
                                                          int mask_mode) {
  for (unsigned i = blockIdx.x * PREP_THREADS + threadIdx.x; i < total; i += gridDim.x * PREP_THREADS) {
    const float x = v[i];
    const bool in = in_mask(x, mask_mode) && x > 0.0f && x < INFINITY;        // a NaN fails x > 0
    u[i] = in ? (float)log((double)x) : 0.0f;
    m[i] = in ? 1 : 0;
  }
}

// ---- histogram -------------------------------------------------------------------------------------------------------
struct BiasHistParams {
  const float* u;
  const uint8_t* m;
  const float* f;
  unsigned long long* hist;      // [BINS] counters, then enc(min) | enc(max) << 32, then the count
  BiasGrid g;
  unsigned total;                // OD * OH * OW
};
struct BiasAt {
  size_t full;
  unsigned d, h, w;              // sample indices
};
__device__ __forceinline__ BiasAt bias_at(const BiasGrid& g, unsigned i) {
  BiasAt a;
  unsigned row = i / g.OW;
  a.w = i - row * g.OW;
  a.h = row % g.OH;
  a.d = row / g.OH;
  a.full = ((size_t)(g.o[0] + g.s[0] * a.d) * g.H + (g.o[1] + g.s[1] * a.h)) * g.W + (g.o[2] + g.s[2] * a.w);
  return a;
}

__global__ __launch_bounds__(PREP_THREADS) void k_bias_hist_clear(unsigned long long* hist) {
  const unsigned i = threadIdx.x;
  if (i < BIAS_BINS) hist[i] = 0ull;
  if (i == BIAS_BINS) hist[i] = 0x00000000ffffffffull;       // min: all ones, max: 0
  if (i == BIAS_BINS + 1) hist[i] = 0ull;
}

__global__ __launch_bounds__(PREP_THREADS) void k_bias_range(BiasHistParams p) {
  float lo = INFINITY, hi = -INFINITY;
  unsigned n = 0;
  for (unsigned i = blockIdx.x * PREP_THREADS + threadIdx.x; i < p.total; i += gridDim.x * PREP_THREADS) {
    const BiasAt a = bias_at(p.g, i);
    if (!p.m[a.full]) continue;
    const float r = p.u[a.full] - p.f[i];
    lo = fminf(lo, r);
    hi = fmaxf(hi, r);
    ++n;
  }
  wave_min_max(lo, hi);
  const unsigned total = wave_sum_all(n);
  if ((threadIdx.x & 63) == 0 && total) {
    unsigned* range = reinterpret_cast<unsigned*>(p.hist + BIAS_BINS);
    atomicMin(range, enc_float(lo));
    atomicMax(range + 1, enc_float(hi));
    atomicAdd(p.hist + BIAS_BINS + 1, (unsigned long long)total);
  }
}

__global__ __launch_bounds__(PREP_THREADS) void k_bias_hist(BiasHistParams p) {
  __shared__ unsigned long long s_hist[BIAS_BINS];       // 64-bit: 2^16 samples of one bin would wrap 32
  for (unsigned i = threadIdx.x; i < BIAS_BINS; i += PREP_THREADS) s_hist[i] = 0ull;
  __syncthreads();
  const unsigned long long packed = p.hist[BIAS_BINS];
  const float lo = dec_float((unsigned)packed), hi = dec_float((unsigned)(packed >> 32));
  if (p.hist[BIAS_BINS + 1] == 0ull || !(hi > lo)) return;       // nothing to count: the host reads min == max
  const double inv = (double)(BIAS_BINS - 1) / ((double)hi - (double)lo);
  for (unsigned i = blockIdx.x * PREP_THREADS + threadIdx.x; i < p.total; i += gridDim.x * PREP_THREADS) {
    const BiasAt a = bias_at(p.g, i);
    if (!p.m[a.full]) continue;
    int k;
    double frac;
    bias_bin(p.u[a.full] - p.f[i], lo, inv, k, frac);
    const unsigned long long q = (unsigned long long)(frac * (double)BIAS_FRAC + 0.5);
    atomicAdd(s_hist + k, (unsigned long long)BIAS_FRAC - q);
    atomicAdd(s_hist + k + 1, q);
  }
  __syncthreads();
  for (unsigned i = threadIdx.x; i < BIAS_BINS; i += PREP_THREADS) {
    const unsigned long long c = s_hist[i];
    if (c) atomicAdd(p.hist + i, c);
  }
}

// ---- fit -------------------------------------------------------------------------------------------------------------
struct BiasFitParams {
  const float* u;
  const uint8_t* m;
  float* f;
  double* part;                  // [slabs][2][P][P]
  double* phi;
  double* Phi;
  double* red;                   // grid_sum_finish: partials
  unsigned* ticket;
  double* sums;
  BiasGrid g;
  int n, P;
  unsigned hchunks;
  float lo;
  double inv;
  double E[BIAS_BINS];
};

__global__ __launch_bounds__(PREP_THREADS) void k_bias_fit_partial(BiasFitParams p) {
  __shared__ float s_e[BIAS_ROWS][BIAS_WC + 1], s_m[BIAS_ROWS][BIAS_WC + 1];
  __shared__ double s_b3[BIAS_WC][BIAS_COLS], s_b2[BIAS_WC][BIAS_COLS];
  __shared__ double s_g[2][BIAS_ROWS][BIAS_COLS];
  __shared__ double s_hw[2][BIAS_ROWS][4];
  __shared__ int s_hk[BIAS_ROWS];
  __shared__ double s_E[BIAS_BINS];
  const BiasGrid& g = p.g;
  const unsigned tid = threadIdx.x, slab = blockIdx.x;
  const unsigned qd = slab / p.hchunks, h0 = (slab - qd * p.hchunks) * BIAS_ROWS;
  const unsigned rows = g.OH - h0 < (unsigned)BIAS_ROWS ? g.OH - h0 : (unsigned)BIAS_ROWS;
  const unsigned d = g.o[0] + g.s[0] * qd;
  for (unsigned i = tid; i < (unsigned)BIAS_BINS; i += PREP_THREADS) s_E[i] = p.E[i];
  if (tid < rows) {
    const BiasW w = bias_weights(g.o[1] + g.s[1] * (h0 + tid), g.H, p.n);
    const double S = sum_sq4(w.w);
    s_hk[tid] = w.k;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s_hw[0][tid][j] = w.w[j] * w.w[j] * w.w[j] / S;
      s_hw[1][tid][j] = w.w[j] * w.w[j];
    }
  }
  __syncthreads();
  const unsigned row = tid & (BIAS_ROWS - 1), cg = tid / BIAS_ROWS;       // columns cg and cg + 8
  double acc_d0 = 0.0, acc_d1 = 0.0, acc_o0 = 0.0, acc_o1 = 0.0;
  for (unsigned w0 = 0; w0 < g.OW; w0 += BIAS_WC) {
    {       // the chunk's banded matrices, dense: thread (x, quarter) writes columns 4 quarter .. 4 quarter + 3 of row x
      const unsigned x = tid & (BIAS_WC - 1), quarter = tid / BIAS_WC;
      const bool live = w0 + x < g.OW;
      const BiasW w = bias_weights(g.o[2] + g.s[2] * (live ? w0 + x : 0u), g.W, p.n);
      const double S = sum_sq4(w.w);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = (int)quarter * 4 + i;
        const double wj = live ? pick4(w.w, c - w.k) : 0.0;
        s_b3[x][c] = wj * wj * wj / S;
        s_b2[x][c] = wj * wj;
      }
    }
#pragma unroll
    for (int it = 0; it < BIAS_ROWS * BIAS_WC / PREP_THREADS; ++it) {
      const unsigned i = tid + it * PREP_THREADS, r_ = i / BIAS_WC, x = i & (BIAS_WC - 1);
      float e = 0.0f, mm = 0.0f;
      if (r_ < rows && w0 + x < g.OW) {
        const size_t full = ((size_t)d * g.H + (g.o[1] + g.s[1] * (h0 + r_))) * g.W + (g.o[2] + g.s[2] * (w0 + x));
        if (p.m[full]) {
          const float r = p.u[full] - p.f[((size_t)qd * g.OH + h0 + r_) * g.OW + w0 + x];
          int k;
          double frac;
          bias_bin(r, p.lo, p.inv, k, frac);
          e = (float)((double)r - (s_E[k] * (1.0 - frac) + s_E[k + 1] * frac));
          mm = 1.0f;
        }
      }
      s_e[r_][x] = e;
      s_m[r_][x] = mm;
    }
    __syncthreads();
#pragma unroll 8
    for (int x = 0; x < BIAS_WC; ++x) {
      const double ev = (double)s_e[row][x], mv = (double)s_m[row][x];
      acc_d0 += s_b3[x][cg] * ev;
      acc_d1 += s_b3[x][cg + 8] * ev;
      acc_o0 += s_b2[x][cg] * mv;
      acc_o1 += s_b2[x][cg + 8] * mv;
    }
    __syncthreads();
  }
  s_g[0][row][cg] = acc_d0;
  s_g[0][row][cg + 8] = acc_d1;
  s_g[1][row][cg] = acc_o0;
  s_g[1][row][cg + 8] = acc_o1;
  __syncthreads();
  const int PP = p.P * p.P;
  if ((int)tid < 2 * PP) {       // the H contraction: thread (q, b, c) walks the slab's rows in order
    const int q = (int)tid / PP, b = ((int)tid - q * PP) / p.P, c = (int)tid % p.P;
    double acc = 0.0;
    for (unsigned r_ = 0; r_ < rows; ++r_) {
      const int j = b - s_hk[r_];
      if (j >= 0 && j < 4) acc += s_hw[q][r_][j] * s_g[q][r_][c];
    }
    p.part[(size_t)slab * 2 * PP + tid] = acc;
  }
}

__global__ __launch_bounds__(PREP_THREADS) void k_bias_fit_lattice(BiasFitParams p) {
  const BiasGrid& g = p.g;
  // a wave per control point: lane i adds the slabs i, i + 64, ... of the point's band in order, then the fixed tree
  const int P = p.P, PP = P * P, lane = threadIdx.x & 63, cell = (int)(blockIdx.x * PREP_WAVES + (threadIdx.x >> 6));
  if (blockIdx.x == 0 && threadIdx.x == 0) *p.ticket = 0u;      // the eval kernel that follows draws tickets from 0
  if (cell >= PP * P) return;                                    // the whole wave
  const int a = cell / PP, bc = cell - a * PP;
  const unsigned slabs = g.OD * p.hchunks;
  double delta = 0.0, omega = 0.0;
  for (unsigned s = lane; s < slabs; s += 64) {
    const BiasW w = bias_weights(g.o[0] + g.s[0] * (s / p.hchunks), g.D, p.n);
    const int j = a - w.k;
    if (j < 0 || j > 3) continue;
    const double wj = pick4(w.w, j);
    const double* at = p.part + (size_t)s * 2 * PP + bc;
    delta += wj * wj * wj / sum_sq4(w.w) * at[0];
    omega += wj * wj * at[PP];
  }
  delta = wave_sum_all(delta);
  omega = wave_sum_all(omega);
  if (lane != 0) return;
  const double v = omega != 0.0 ? delta / omega : 0.0;
  p.phi[cell] = v;
  p.Phi[cell] += v;
}

// Lane c < P of a wave: sum_a sum_b wd[a] wh[b] lat[kd + a][kh + b][c], the row coefficient c of a P^3 lattice.
__device__ __forceinline__ double bias_row_coeff(const double* lat, int P, const BiasW& wd, const BiasW& wh, int c) {
  double r = 0.0;
  if (c < P) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) r += wd.w[a] * wh.w[b] * lat[((wd.k + a) * P + wh.k + b) * P + c];
  }
  return r;
}
// sum_j ww[j] coeff[lane base + kw + j]; every lane of the wave calls it.
__device__ __forceinline__ double bias_row_eval(double coeff, int base, const BiasW& ww) {
  double v = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) v += ww.w[j] * __shfl(coeff, base + ww.k + j, 64);
  return v;
}

__global__ __launch_bounds__(PREP_THREADS) void k_bias_fit_eval(BiasFitParams p) {
  __shared__ double s_phi[BIAS_MAX_P * BIAS_MAX_P * BIAS_MAX_P];
  __shared__ double s_red[2 * 16];
  __shared__ int s_last;
  const BiasGrid& g = p.g;
  const int P = p.P, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < P * P * P; i += PREP_THREADS) s_phi[i] = p.phi[i];
  __syncthreads();
  double v[2] = {0.0, 0.0};
  const unsigned nrows = g.OD * g.OH;
  for (unsigned rowi = blockIdx.x * PREP_WAVES + wave; rowi < nrows; rowi += gridDim.x * PREP_WAVES) {
    const unsigned qd = rowi / g.OH, qh = rowi - qd * g.OH;
    const BiasW wd = bias_weights(g.o[0] + g.s[0] * qd, g.D, p.n), wh = bias_weights(g.o[1] + g.s[1] * qh, g.H, p.n);
    const double coeff = bias_row_coeff(s_phi, P, wd, wh, lane);
    const size_t full0 = ((size_t)(g.o[0] + g.s[0] * qd) * g.H + (g.o[1] + g.s[1] * qh)) * g.W + g.o[2];
    for (unsigned x0 = 0; x0 < g.OW; x0 += 64) {         // the whole wave walks: the shuffles need every lane
      const unsigned x = x0 + lane;
      const bool live = x < g.OW;
      const BiasW ww = bias_weights(g.o[2] + g.s[2] * (live ? x : 0u), g.W, p.n);
      const double df = bias_row_eval(coeff, 0, ww);
      if (live) {
        const size_t si = (size_t)rowi * g.OW + x;
        p.f[si] = p.f[si] + (float)df;
        if (p.m[full0 + (size_t)g.s[2] * x]) {
          const double ex = exp(df);
          v[0] += ex;
          v[1] += ex * ex;
        }
      }
    }
  }
  grid_sum_finish<2>(v, p.red, p.ticket, p.sums, s_red, &s_last);
}

// ---- apply -----------------------------------------------------------------------------------------------------------
struct BiasApplyParams {
  const float* v;
  const uint8_t* m;              // may be null: no range
  const double* Phi;             // BIAS_LATTICE doubles
  float* y;
  unsigned* range;               // enc(min), enc(max) of exp(f) over m
  unsigned D, H, W;
};

__global__ void k_bias_range_clear(unsigned* range) {
  range[0] = 0xffffffffu;
  range[1] = 0u;
}

__global__ __launch_bounds__(PREP_THREADS) void k_bias_apply(BiasApplyParams p) {
  __shared__ double s_lat[BIAS_LATTICE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < BIAS_LATTICE; i += PREP_THREADS) s_lat[i] = p.Phi[i];
  __syncthreads();
  // lane i < 27 holds row coefficient c of level l: the levels side by side at lanes 0, 4, 9, 16
  int level = -1, c = 0, at = 0;
  {
    int base = 0, off = 0;
#pragma unroll
    for (int l = 0; l < BIAS_LEVELS; ++l) {
      const int P = (1 << l) + 3;
      if (lane >= base && lane < base + P) {
        level = l;
        c = lane - base;
        at = off;
      }
      base += P;
      off += P * P * P;
    }
  }
  float lo = INFINITY, hi = -INFINITY;
  const unsigned nrows = p.D * p.H;
  for (unsigned rowi = blockIdx.x * PREP_WAVES + wave; rowi < nrows; rowi += gridDim.x * PREP_WAVES) {
    const unsigned d = rowi / p.H, h = rowi - d * p.H;
    double coeff = 0.0;
    if (level >= 0) {
      const int n = 1 << level;
      coeff = bias_row_coeff(s_lat + at, n + 3, bias_weights(d, p.D, n), bias_weights(h, p.H, n), c);
    }
    const size_t row0 = (size_t)rowi * p.W;
    for (unsigned x0 = 0; x0 < p.W; x0 += 64) {
      const unsigned x = x0 + lane;
      const bool live = x < p.W;
      double f = 0.0;
      int base = 0;
#pragma unroll
      for (int l = 0; l < BIAS_LEVELS; ++l) {
        f += bias_row_eval(coeff, base, bias_weights(live ? x : 0u, p.W, 1 << l));
        base += (1 << l) + 3;
      }
      if (live) {
        const double ex = exp(f);
        p.y[row0 + x] = (float)((double)p.v[row0 + x] / ex);
        if (p.m && p.m[row0 + x]) {
          lo = fminf(lo, (float)ex);
          hi = fmaxf(hi, (float)ex);
        }
      }
    }
  }
  if (p.m) {
    wave_min_max(lo, hi);
    if (lane == 0 && lo <= hi) {
      atomicMin(p.range, enc_float(lo));
      atomicMax(p.range + 1, enc_float(hi));
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
// The sample geometry of (stride, offset), or false: a stride below 1, or an offset outside the axis.
static bool bias_grid(int D, int H, int W, const int* stride, const int* offset, BiasGrid& g) {
  if (!stride || !offset || !prep_fits(1, D, H, W)) return false;
  const int n[3] = {D, H, W};
  unsigned o[3];
  for (int a = 0; a < 3; ++a) {
    if (stride[a] < 1 || offset[a] < 0 || offset[a] >= n[a]) return false;
    g.s[a] = (unsigned)stride[a];
    g.o[a] = (unsigned)offset[a];
    o[a] = (unsigned)((n[a] - offset[a] + stride[a] - 1) / stride[a]);
  }
  g.D = D; g.H = H; g.W = W; g.OD = o[0]; g.OH = o[1]; g.OW = o[2];
  return true;
}
static inline unsigned bias_hchunks(const BiasGrid& g) { return (g.OH + BIAS_ROWS - 1) / BIAS_ROWS; }
static inline size_t bias_part_bytes(const BiasGrid& g) {
  return sizeof(double) * 2 * BIAS_MAX_P * BIAS_MAX_P * (size_t)g.OD * bias_hchunks(g);
}
constexpr size_t BIAS_RED_BYTES = sizeof(double) * 2 * PREP_MAX_BLOCKS;

}  // namespace effq
using namespace effq;

extern "C" {

int effq_prep_bias_log(const float* v, int D, int H, int W, int mask_mode, float* u, unsigned char* m, void* stream) {
  EFFQ_CHECK_ARG(v && u && m && prep_fits(1, D, H, W) && aligned_to(v, 4) && aligned_to(u, 4));
  EFFQ_CHECK_ARG(mask_mode == EFFQ_PREP_MASK_NONZERO || mask_mode == EFFQ_PREP_MASK_ALL);
  const unsigned total = (unsigned)((size_t)D * H * W);
  hipLaunchKernelGGL(k_bias_log, dim3(prep_grid(total)), dim3(PREP_THREADS), 0, as_stream(stream), v, u, m, total,
                     mask_mode);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_prep_bias_hist(const float* u, const unsigned char* m, const float* f, int D, int H, int W, const int* stride,
                        const int* offset, unsigned long long* hist, void* stream) {
  BiasHistParams p;
  EFFQ_CHECK_ARG(u && m && f && hist && bias_grid(D, H, W, stride, offset, p.g));
  EFFQ_CHECK_ARG(aligned_to(u, 4) && aligned_to(f, 4) && aligned_to(hist, 8));
  p.u = u; p.m = m; p.f = f; p.hist = hist;
  p.total = p.g.OD * p.g.OH * p.g.OW;
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_bias_hist_clear, dim3(1), dim3(PREP_THREADS), 0, st, hist);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bias_range, dim3(prep_grid(p.total)), dim3(PREP_THREADS), 0, st, p);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bias_hist, dim3(prep_grid(p.total)), dim3(PREP_THREADS), 0, st, p);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

size_t effq_bias_fit_ws_bytes(int D, int H, int W, const int* stride, const int* offset) {
  BiasGrid g;
  if (!bias_grid(D, H, W, stride, offset, g)) return 0;
  return bias_part_bytes(g) + BIAS_RED_BYTES + 256;
}

int effq_prep_bias_fit(const float* u, const unsigned char* m, float* f, int D, int H, int W, const int* stride,
                       const int* offset, int level, float lo, float hi, const double* E, double* phi, double* Phi,
                       double* sums, void* ws, size_t ws_bytes, void* stream) {
  BiasGrid g;
  EFFQ_CHECK_ARG(u && m && f && E && phi && Phi && sums && ws && bias_grid(D, H, W, stride, offset, g));
  EFFQ_CHECK_ARG(level >= 0 && level < BIAS_LEVELS && isfinite(lo) && isfinite(hi) && hi > lo);
  EFFQ_CHECK_ARG(aligned_to(u, 4) && aligned_to(f, 4) && aligned_to(phi, 8) && aligned_to(Phi, 8) && aligned_to(sums, 8) &&
                 aligned_to(ws, 8));
  for (int i = 0; i < BIAS_BINS; ++i) EFFQ_CHECK_ARG(isfinite(E[i]));
  EFFQ_CHECK_WS(ws_bytes, bias_part_bytes(g) + BIAS_RED_BYTES + 256);
  BiasFitParams q;
  q.u = u; q.m = m; q.f = f; q.phi = phi; q.Phi = Phi; q.sums = sums; q.g = g;
  q.part = reinterpret_cast<double*>(ws);
  q.red = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + bias_part_bytes(g));
  q.ticket = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(q.red) + BIAS_RED_BYTES);
  q.n = 1 << level; q.P = q.n + 3; q.hchunks = bias_hchunks(g);
  q.lo = lo; q.inv = (double)(BIAS_BINS - 1) / ((double)hi - (double)lo);
  for (int i = 0; i < BIAS_BINS; ++i) q.E[i] = E[i];
  const hipStream_t st = as_stream(stream);
  const unsigned cells = (unsigned)(q.P * q.P * q.P), nrows = g.OD * g.OH;
  hipLaunchKernelGGL(k_bias_fit_partial, dim3(g.OD * q.hchunks), dim3(PREP_THREADS), 0, st, q);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bias_fit_lattice, dim3((cells + PREP_WAVES - 1) / PREP_WAVES), dim3(PREP_THREADS), 0, st, q);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bias_fit_eval, dim3(prep_grid((size_t)(nrows + PREP_WAVES - 1) / PREP_WAVES * PREP_THREADS)),
                     dim3(PREP_THREADS), 0, st, q);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

int effq_prep_bias_apply(const float* v, const unsigned char* m, int D, int H, int W, const double* Phi, float* y,
                         unsigned* range, void* stream) {
  EFFQ_CHECK_ARG(v && Phi && y && prep_fits(1, D, H, W) && aligned_to(v, 4) && aligned_to(y, 4) && aligned_to(Phi, 8));
  EFFQ_CHECK_ARG((m == nullptr) == (range == nullptr) && aligned_to(range, 4));
  BiasApplyParams p;
  p.v = v; p.m = m; p.Phi = Phi; p.y = y; p.range = range; p.D = D; p.H = H; p.W = W;
  const hipStream_t st = as_stream(stream);
  if (range) {
    hipLaunchKernelGGL(k_bias_range_clear, dim3(1), dim3(1), 0, st, range);
    EFFQ_LAUNCH_CHECK();
  }
  const size_t nrows = (size_t)D * H;
  hipLaunchKernelGGL(k_bias_apply, dim3(prep_grid((nrows + PREP_WAVES - 1) / PREP_WAVES * PREP_THREADS)),
                     dim3(PREP_THREADS), 0, st, p);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
