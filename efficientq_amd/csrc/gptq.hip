// One-pass sequential rounding with error feedback (OBQ / GPTQ, Babai's nearest plane) for the layer calibration:
// the fp64 factor of H = A0 + eta I and the sweep over the columns.  The rule is efficientq_amd/gptq.py.
//
// H = P P^T with P upper triangular is the Cholesky factorisation of the index-reversed matrix: with i' = n - 1 - i,
// Hr[i'][j'] = H[i][j] = (L L^T)[i'][j'] and P[i][j] = L[i'][j'].  Everything here works on L, in REVERSED indices:
//   factor buffer = L, npad x npad doubles row-major (npad = n rounded up to 64; identity on the padding i' >= n, zeros
//   above the diagonal), then GQ_HDR doubles of header whose first 32-bit word is the "not positive definite" flag.
// The sweep visits the columns j = 0 .. n-1 of the rule, i.e. j' = n-1 .. 0: the 64-blocks of L from the last to the
// first and the rows of a block from the bottom up; the padding lies at the start of the walk and contributes nothing.
//
// effq_gptq_chol: blocked right-looking factorisation, three launches per 64-block k:
//   k_gq_diag   one workgroup: the 64 x 64 diagonal block is factored in LDS (a pivot <= 0 or not finite sets the flag),
//               its triangular inverse is formed in LDS by forward substitution, one column per lane;
//   k_gq_panel  L_ik = A_ik L_kk^-T as a 64^3 product on the fp64 matrix cores, one workgroup per block row i > k;
//   k_gq_trail  A_ij -= L_ik L_jk^T for the tiles i >= j > k of the lower triangle only, one workgroup per tile, both
//               operands staged in LDS (the second one read transposed), v_mfma_f64_16x16x4_f64.
// effq_gptq_sweep: two launches per 64-block B, no host read in between:
//   k_gq_block  one wave per output row, four rows per workgroup; the diagonal block of L in LDS, lane l holds s, u* and
//               the result of column 64 B + l; the 64 dependent steps broadcast delta_j with v_readlane;
//   k_gq_strail S[:, 0 .. 64 B) += Delta_B (c2 x 64) * L[B, 0 .. 64 B) on the fp64 matrix cores, the 16 values of the L
//               operand of a wave held in registers across its row tiles.
// Every kernel reads the flag first and returns when it is set; no kernel waits for another or loops on memory.
#include <math.h>
#include "common.h"
#include "fp_level.h"
#include "gptq.h"

namespace effq {

constexpr int GQ_LDA = 66;        // LDS leading dimension (doubles) of the matrix-core operands
constexpr int GQ_HDR = 32;        // doubles behind L: [0] = the flag (int32)
constexpr int GQ_LDT = 65;        // LDS leading dimension of the diagonal block while it is factored

// L (reversed indices) = the lower triangle of A0 + eta I, identity on the padding, zeros above the diagonal; flag = 0
__global__ __launch_bounds__(256) void k_gq_build(const float* __restrict__ A0, int n, int npad, double eta,
                                                  double* __restrict__ L, int* __restrict__ flag) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *flag = 0;
  const size_t tot = (size_t)npad * npad;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += stride) {
    const int i = (int)(e / npad), j = (int)(e % npad);
    double v = 0.0;
    if (j <= i) {
      if (i < n)
        v = (double)A0[(size_t)(n - 1 - i) * n + (n - 1 - j)] + (i == j ? eta : 0.0);
      else if (i == j)
        v = 1.0;
    }
    L[e] = v;
  }
}

// The diagonal block kb: L_kk in place, Winv = L_kk^-1 (64 x 64, row-major)
__global__ __launch_bounds__(256) void k_gq_diag(double* __restrict__ L, int npad, int kb, double* __restrict__ Winv,
                                                 int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) double gq_sm[];
  double* T = gq_sm;                       // [64][GQ_LDT] the block, then its factor
  double* X = gq_sm + GQ_B * GQ_LDT;       // [64][GQ_LDT] the inverse of the factor
  if (*flag != 0) return;
  const int tid = threadIdx.x;
  for (int e = tid; e < GQ_B * GQ_B; e += 256) {
    const int r = e >> 6, c = e & 63;
    T[r * GQ_LDT + c] = L[(size_t)(kb + r) * npad + kb + c];
    X[r * GQ_LDT + c] = 0.0;
  }
  __syncthreads();
  bool bad = false;
  for (int p = 0; p < GQ_B; ++p) {
    const double d = T[p * GQ_LDT + p];      // the same word in every thread: the branch below is uniform
    if (!(d > 0.0) || !(d <= 1.79e308)) {
      bad = true;
      break;
    }
    const double l = sqrt(d);
    __syncthreads();
    if (tid < GQ_B && tid >= p) T[tid * GQ_LDT + p] = (tid == p) ? l : T[tid * GQ_LDT + p] / l;
    __syncthreads();
    for (int e = tid; e < GQ_B * GQ_B; e += 256) {
      const int i = e >> 6, j = e & 63;
      if (j > p && i >= j) T[i * GQ_LDT + j] -= T[i * GQ_LDT + p] * T[j * GQ_LDT + p];
    }
    __syncthreads();
  }
  if (bad) {
    if (tid == 0) *flag = 1;
    return;
  }
  // X = T^-1, column c by lane c: X[c][c] = 1 / T[c][c], X[i][c] = -(sum_{c <= k < i} T[i][k] X[k][c]) / T[i][i]
  if (tid < GQ_B) {
    const int c = tid;
    X[c * GQ_LDT + c] = 1.0 / T[c * GQ_LDT + c];
    for (int i = c + 1; i < GQ_B; ++i) {
      double s = 0.0;
      for (int k = c; k < i; ++k) s += T[i * GQ_LDT + k] * X[k * GQ_LDT + c];
      X[i * GQ_LDT + c] = -s / T[i * GQ_LDT + i];
    }
  }
  __syncthreads();
  for (int e = tid; e < GQ_B * GQ_B; e += 256) {
    const int r = e >> 6, c = e & 63;
    L[(size_t)(kb + r) * npad + kb + c] = (c <= r) ? T[r * GQ_LDT + c] : 0.0;
    Winv[e] = X[r * GQ_LDT + c];
  }
}

// acc (one 32 x 32 quadrant per wave) += As * Bs^T: both 64 x 64 tiles lie row-major in LDS, A[m][k] = As[m * GQ_LDA + k]
// and B[k][n] = Bs[n * GQ_LDA + k] (the second operand is read transposed)
__device__ __forceinline__ void gq_tile_mma(const double* As, const double* Bs, gq_f64x4 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll 4
  for (int ks = 0; ks < GQ_B / 4; ++ks) {
    double a[2], b[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) a[mi] = As[(wr * 32 + mi * 16 + lr) * GQ_LDA + ks * 4 + lk];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) b[ni] = Bs[(wc * 32 + ni * 16 + lr) * GQ_LDA + ks * 4 + lk];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
  }
}

// L_ik = A_ik * L_kk^-T for the block row i = kb / 64 + 1 + blockIdx.x
__global__ __launch_bounds__(256) void k_gq_panel(double* __restrict__ L, int npad, int kb,
                                                  const double* __restrict__ Winv, const int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) double gq_sm[];
  double* As = gq_sm;                      // A_ik
  double* Bs = gq_sm + GQ_B * GQ_LDA;      // L_kk^-1
  if (*flag != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1, lr = lane & 15, lk = lane >> 4;
  double* Ab = L + (size_t)(kb + GQ_B * (1 + (int)blockIdx.x)) * npad + kb;
  for (int e = tid; e < GQ_B * GQ_B; e += 256) {
    const int r = e >> 6, c = e & 63;
    As[r * GQ_LDA + c] = Ab[(size_t)r * npad + c];
    Bs[r * GQ_LDA + c] = Winv[e];
  }
  __syncthreads();
  gq_f64x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[mi][ni][r] = 0.0;
  gq_tile_mma(As, Bs, acc);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        Ab[(size_t)(wr * 32 + mi * 16 + lk + 4 * r) * npad + wc * 32 + ni * 16 + lr] = acc[mi][ni][r];
}

// A_ij -= L_ik L_jk^T for tile blockIdx.x of the lower triangle behind block k (i >= j > k, counted row by row)
__global__ __launch_bounds__(256) void k_gq_trail(double* __restrict__ L, int npad, int kb, const int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) double gq_sm[];
  double* As = gq_sm;                      // -L_ik
  double* Bs = gq_sm + GQ_B * GQ_LDA;      // L_jk
  if (*flag != 0) return;
  const int t = (int)blockIdx.x;
  int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  if ((i + 1) * (i + 2) / 2 <= t) ++i;        // the square root rounded down across an exact triangle number ...
  if (i * (i + 1) / 2 > t) --i;               // ... or up
  const int j = t - i * (i + 1) / 2;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1, lr = lane & 15, lk = lane >> 4;
  const size_t r0 = (size_t)kb + GQ_B * (size_t)(1 + i), c0 = (size_t)kb + GQ_B * (size_t)(1 + j);
  const double* Li = L + r0 * npad + kb;
  const double* Lj = L + c0 * npad + kb;
  for (int e = tid; e < GQ_B * GQ_B; e += 256) {
    const int r = e >> 6, c = e & 63;
    As[r * GQ_LDA + c] = -Li[(size_t)r * npad + c];
    Bs[r * GQ_LDA + c] = Lj[(size_t)r * npad + c];
  }
  double* Cb = L + (r0 + wr * 32) * npad + c0 + wc * 32;
  gq_f64x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[mi][ni][r] = Cb[(size_t)(mi * 16 + lk + 4 * r) * npad + ni * 16 + lr];
  __syncthreads();
  gq_tile_mma(As, Bs, acc);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) Cb[(size_t)(mi * 16 + lk + 4 * r) * npad + ni * 16 + lr] = acc[mi][ni][r];
}

// ---- the sweep ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gq_zero(double* __restrict__ p, size_t count, const int* __restrict__ flag) {
  if (*flag != 0) return;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += stride) p[e] = 0.0;
}

struct GqSweep {
  const double* L;
  const float *uw, *ub;        // u*: weights [c2][nw], bias [c2] (or NULL)
  const double* alpha;         // 1 or c2 scales
  double *S, *Delta;           // [c2pad][npad], [c2pad][64]
  float *G, *b;
  uint8_t* ids;
  double* err;
  int32_t* row_flag;
  int n, npad, nw, c2, has_bias, per_row, levels, first;
};

// Block B of the sweep for the rows 4 blockIdx.x .. + 3: the rule of gptq.py on the columns j' = 64 B + 63 .. 64 B
__global__ __launch_bounds__(64 * GQ_ROWS) void k_gq_block(const GqSweep p, int B) {
  __shared__ double Lb[GQ_B * GQ_B];
  const int* flag = reinterpret_cast<const int*>(p.L + (size_t)p.npad * p.npad);
  if (*flag != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const size_t kb = (size_t)B * GQ_B;
  for (int e = tid; e < GQ_B * GQ_B; e += 64 * GQ_ROWS) Lb[e] = p.L[(kb + (e >> 6)) * p.npad + kb + (e & 63)];
  __syncthreads();
  const int r = (int)blockIdx.x * GQ_ROWS + wid;
  if (r >= p.c2) return;
  const double a = p.alpha[p.per_row ? r : 0];
  const bool row_ok = a > 0.0 && a <= 1.79e308;
  if (lane == 0 && p.first) p.row_flag[r] = row_ok ? 0 : 1;
  if (!row_ok) {                      // nothing of this row is written; it feeds nothing back
    p.Delta[(size_t)r * GQ_B + lane] = 0.0;
    return;
  }
  const int jr = (int)kb + lane;                    // reversed column of this lane
  const bool valid = jr < p.n;
  const int j = p.n - 1 - jr;                       // column of the rule
  const bool is_bias = p.has_bias && jr == 0;
  double u = 0.0;
  if (valid) u = is_bias ? (double)p.ub[r] : (double)p.uw[(size_t)r * p.nw + j];
  double s = p.S[(size_t)r * p.npad + jr];
  const double d = 2.0 / (double)(p.levels - 1);
  double q_mine = 0.0, idx_mine = 0.0, e_mine = 0.0;
  const int top = (p.n - (int)kb < GQ_B) ? p.n - (int)kb : GQ_B;     // the padding of the last block takes no step
  for (int jj = top - 1; jj >= 0; --jj) {
    const double ljj = Lb[jj * GQ_B + jj];
    const double t = u - s / ljj;                   // every lane computes, lane jj's value is the step's
    double idx = 0.0, q = t;
    if (!is_bias) q = a * disc64(t, a, -1.0, 1.0, d, &idx);
    const double e = ljj * (q - t);
    if (lane == jj) {
      q_mine = q;
      idx_mine = idx;
      e_mine = e * e;
    }
    const double dj = gq_readlane(q - u, jj);
    if (lane < jj) s += dj * Lb[jj * GQ_B + lane];
  }
  p.Delta[(size_t)r * GQ_B + lane] = valid ? q_mine - u : 0.0;
  if (valid) {
    if (is_bias) {
      p.b[r] = (float)q_mine;
    } else {
      p.G[(size_t)r * p.nw + j] = gq_weight_f32(a, idx_mine, d, p.per_row);      // (gptq.h: the restore arithmetic)
      if (p.ids != nullptr) p.ids[(size_t)r * p.nw + j] = (uint8_t)idx_mine;
    }
  }
  const double es = wave_sum_f64_dpp(e_mine);
  if (lane == 0) p.err[r] = p.first ? es : p.err[r] + es;
}

// S[:, 0 .. 64 B) += Delta (c2pad x 64) * L[64 B .. 64 B + 63, 0 .. 64 B): blockIdx.x = column block, blockIdx.y = group
// of 64 rows; wave w takes the columns 16 w .. 16 w + 15 of the block and every 16-row tile of the group
__global__ __launch_bounds__(256) void k_gq_strail(const GqSweep p, int B, int c2pad) {
  const int* flag = reinterpret_cast<const int*>(p.L + (size_t)p.npad * p.npad);
  if (*flag != 0) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  const size_t col = (size_t)blockIdx.x * GQ_B + wid * 16 + lr;
  const double* Lr = p.L + (size_t)B * GQ_B * p.npad + col;
  double b[GQ_B / 4];
#pragma unroll
  for (int ks = 0; ks < GQ_B / 4; ++ks) b[ks] = Lr[(size_t)(ks * 4 + lk) * p.npad];
  for (int mi = 0; mi < 4; ++mi) {
    const int row0 = ((int)blockIdx.y * 4 + mi) * 16;
    if (row0 >= c2pad) break;
    const double* Dr = p.Delta + (size_t)(row0 + lr) * GQ_B + lk;
    double* Sb = p.S + (size_t)(row0 + lk) * p.npad + col;
    gq_f64x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = Sb[(size_t)(4 * r) * p.npad];
#pragma unroll
    for (int ks = 0; ks < GQ_B / 4; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Dr[ks * 4], b[ks], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) Sb[(size_t)(4 * r) * p.npad] = acc[r];
  }
}

}  // namespace effq

using namespace effq;

extern "C" {

size_t effq_gptq_factor_bytes(int n) {
  if (n < 1 || n > GQ_MAX_N) return 0;
  const size_t npad = (size_t)round_up(n, GQ_B);
  return (npad * npad + GQ_HDR) * sizeof(double);
}

size_t effq_gptq_chol_ws_bytes(int n) { return (n < 1 || n > GQ_MAX_N) ? 0 : GQ_B * GQ_B * sizeof(double) + 256; }

size_t effq_gptq_ws_bytes(int c2, int n) {
  if (n < 1 || n > GQ_MAX_N || c2 < 1) return 0;
  const size_t npad = (size_t)round_up(n, GQ_B), c2pad = (size_t)round_up(c2, 16);
  return c2pad * (npad + GQ_B) * sizeof(double) + 256;
}

int effq_gptq_plan_query(int c2, int n, int* nblk, int* chol_launches, int* chol_tiles, int* sweep_launches,
                         int* block_grid, int* trail_gy) {
  EFFQ_CHECK_ARG(c2 >= 1 && n >= 1 && n <= GQ_MAX_N && nblk && chol_launches && chol_tiles && sweep_launches &&
                 block_grid && trail_gy);
  const int nb = round_up(n, GQ_B) / GQ_B;
  *nblk = nb;
  *chol_launches = 1 + nb + 2 * (nb - 1);       // build, a diagonal block per step, panel + update behind all but the last
  *chol_tiles = (nb - 1) * nb / 2;              // tiles of the first trailing update
  *sweep_launches = 1 + nb + (nb - 1);
  *block_grid = (c2 + GQ_ROWS - 1) / GQ_ROWS;
  *trail_gy = (round_up(c2, 16) + 63) / 64;
  return EFFQ_OK;
}

int effq_gptq_chol(const float* A0, double eta, int n, double* P, size_t p_bytes, void* ws, size_t ws_bytes,
                   int read_flag, void* stream) {
  EFFQ_CHECK_ARG(A0 && P && ws && n >= 1 && n <= GQ_MAX_N);
  EFFQ_CHECK_ARG(eta > 0.0 && eta <= 1.79e308);
  EFFQ_CHECK_ARG(p_bytes >= effq_gptq_factor_bytes(n));
  EFFQ_CHECK_WS(ws_bytes, effq_gptq_chol_ws_bytes(n));
  const int npad = round_up(n, GQ_B), nb = npad / GQ_B;
  int* flag = reinterpret_cast<int*>(P + (size_t)npad * npad);
  double* Winv = reinterpret_cast<double*>(ws);
  hipStream_t st = as_stream(stream);
  constexpr size_t lds_diag = 2 * GQ_B * GQ_LDT * sizeof(double), lds_mma = 2 * GQ_B * GQ_LDA * sizeof(double);
  EFFQ_HIP(raise_lds_limit<k_gq_diag>(lds_diag));
  EFFQ_HIP(raise_lds_limit<k_gq_panel>(lds_mma));
  EFFQ_HIP(raise_lds_limit<k_gq_trail>(lds_mma));
  size_t g = ((size_t)npad * npad + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(k_gq_build, dim3((unsigned)g), dim3(256), 0, st, A0, n, npad, eta, P, flag);
  EFFQ_LAUNCH_CHECK();
  for (int k = 0; k < nb; ++k) {
    const int kb = k * GQ_B, m = nb - 1 - k;
    hipLaunchKernelGGL(k_gq_diag, dim3(1), dim3(256), lds_diag, st, P, npad, kb, Winv, flag);
    if (m > 0) {
      hipLaunchKernelGGL(k_gq_panel, dim3(m), dim3(256), lds_mma, st, P, npad, kb, Winv, flag);
      hipLaunchKernelGGL(k_gq_trail, dim3(m * (m + 1) / 2), dim3(256), lds_mma, st, P, npad, kb, flag);
    }
    EFFQ_LAUNCH_CHECK();
  }
  if (read_flag) {
    int h = 0;
    EFFQ_HIP(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    EFFQ_HIP(hipStreamSynchronize(st));
    if (h != 0) {
      set_error("effq_gptq_chol: A0 + eta I is not positive definite (a pivot <= 0 or not finite)");
      return EFFQ_ERR_NOT_SPD;
    }
  }
  return EFFQ_OK;
}

int effq_gptq_sweep(const double* P, int n, const float* uw, const float* ub, int c2, int has_bias, const double* alpha,
                    int per_row, int levels, float* G, float* b, uint8_t* ids, double* err, int32_t* row_flag, void* ws,
                    size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(P && alpha && err && row_flag && ws && n >= 1 && n <= GQ_MAX_N && c2 >= 1);
  EFFQ_CHECK_ARG(levels >= 2 && levels <= FP_LEVELS_MAX);
  const int hb = has_bias ? 1 : 0, nw = n - hb;
  EFFQ_CHECK_ARG(!hb || (ub != nullptr && b != nullptr));
  EFFQ_CHECK_ARG(nw == 0 || (uw != nullptr && G != nullptr));
  EFFQ_CHECK_WS(ws_bytes, effq_gptq_ws_bytes(c2, n));
  const int npad = round_up(n, GQ_B), nb = npad / GQ_B, c2pad = round_up(c2, 16);
  GqSweep p;
  p.L = P; p.uw = uw; p.ub = ub; p.alpha = alpha;
  p.S = reinterpret_cast<double*>(ws);
  p.Delta = p.S + (size_t)c2pad * npad;
  p.G = G; p.b = b; p.ids = ids; p.err = err; p.row_flag = row_flag;
  p.n = n; p.npad = npad; p.nw = nw; p.c2 = c2; p.has_bias = hb; p.per_row = per_row ? 1 : 0; p.levels = levels;
  p.first = 1;
  hipStream_t st = as_stream(stream);
  const int* flag = reinterpret_cast<const int*>(P + (size_t)npad * npad);
  const size_t count = (size_t)c2pad * (npad + GQ_B);
  size_t g = (count + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(k_gq_zero, dim3((unsigned)g), dim3(256), 0, st, p.S, count, flag);
  EFFQ_LAUNCH_CHECK();
  for (int B = nb - 1; B >= 0; --B) {
    hipLaunchKernelGGL(k_gq_block, dim3((c2 + GQ_ROWS - 1) / GQ_ROWS), dim3(64 * GQ_ROWS), 0, st, p, B);
    if (B > 0) hipLaunchKernelGGL(k_gq_strail, dim3(B, (c2pad + 63) / 64), dim3(256), 0, st, p, B, c2pad);
    EFFQ_LAUNCH_CHECK();
    p.first = 0;
  }
  return EFFQ_OK;
}

}  // extern "C"
