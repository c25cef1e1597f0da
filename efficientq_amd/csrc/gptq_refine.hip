// Coordinate-descent passes behind the sweep of gptq.hip (the "greedy passes" of LDLQ, the local search of OBQ): every
// column of every output row is revisited in the rule's order and moved to the grid value next to its conditional
// minimiser when that lowers the row's error.  The rule is refine_host of efficientq_amd/gptq.py.
//
// Everything here works in NATURAL indices on H = A0 + eta I itself, read from the fp32 A0 (its upper triangle; the mirror
// element serves the other one) and converted in registers: no fp64 copy of H is made, a pass streams n^2 floats once.
// State per output row, fp64, in the workspace: q (the current values, npad wide), g = (q - u*) H, and per 64-block the
// Delta of the block's columns.
//   k_gr_init    q from the level ids and the bias the sweep left, D = q - u*, g = 0, the move counts = 0;
//   k_gr_update  g[:, C] += Dl (c2pad x 64) * H[B, C] for every column block C (but B itself unless asked for) on
//                v_mfma_f64_16x16x4_f64: wave w owns 16 columns of C and keeps its 16 H values in registers across the
//                row tiles.  Right of the block (C > B) the lanes read A0's rows directly, 16 consecutive floats each; left
//                of it (and on B itself) the element needed is the mirror one, so the 64 x 64 tile of A0 is read with
//                coalesced rows into LDS and read out transposed.  With Dl = D and B included this builds the first g;
//   k_gr_block   one wave per output row, four rows per workgroup share H[B, B] in LDS (built from A0, mirrored, eta on
//                the diagonal); lane l holds q and g of column 64 B + l (u* is inside g); the 64 dependent steps broadcast the accepted
//                delta with v_readlane and every lane, on both sides of the pivot, updates its g;
//   k_gr_err     one wave per row: err = sum_j g_j (q_j - u*_j).
// Every kernel reads the factor's "not positive definite" word first and returns when it is set; a row whose flag is set
// writes nothing.  No kernel waits for another or loops on memory, nothing is read back.
#include <math.h>
#include "common.h"
#include "fp_level.h"
#include "gptq.h"

namespace effq {

constexpr int GR_LDT = 65;        // LDS leading dimension (floats) of the tile that is read out transposed
constexpr int GR_MAX_PASSES = 16;

struct GrArgs {
  const float *A0, *uw, *ub;   // u*: weights [c2][nw], bias [c2] (or NULL)
  const double* alpha;         // 1 or c2 scales
  const int32_t* row_flag;
  const int* pd_flag;
  double *g, *q, *D;           // [c2pad][npad] each
  double* Delta;               // [c2pad][64]
  float *G, *b;
  uint8_t* ids;
  double* err;
  int32_t* moves;
  double eta;
  int n, npad, nw, c2, c2pad, has_bias, per_row, levels;
};

__device__ __forceinline__ bool gr_row_ok(const GrArgs& p, int r, double* a) {
  *a = p.alpha[p.per_row ? r : 0];
  return p.row_flag[r] == 0 && *a > 0.0 && *a <= 1.79e308;
}

__device__ __forceinline__ double gr_ustar(const GrArgs& p, int r, int c) {
  return (p.has_bias && c == p.n - 1) ? (double)p.ub[r] : (double)p.uw[(size_t)r * p.nw + c];
}

__global__ __launch_bounds__(256) void k_gr_init(const GrArgs p) {
  if (*p.pd_flag != 0) return;
  const size_t tot = (size_t)p.c2pad * p.npad;
  const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const double d = 2.0 / (double)(p.levels - 1);
  for (size_t e = first; e < tot; e += stride) {
    const int r = (int)(e / p.npad), c = (int)(e % p.npad);
    double q = 0.0, dd = 0.0, a;
    if (r < p.c2 && c < p.n && gr_row_ok(p, r, &a)) {
      q = (p.has_bias && c == p.n - 1) ? (double)p.b[r] : a * ((double)p.ids[(size_t)r * p.nw + c] * d + -1.0);
      dd = q - gr_ustar(p, r, c);
    }
    p.g[e] = 0.0;
    p.q[e] = q;
    p.D[e] = dd;
  }
  for (size_t e = first; e < (size_t)p.c2pad * GQ_B; e += stride) p.Delta[e] = 0.0;
  double a;
  for (size_t r = first; r < (size_t)p.c2; r += stride)
    if (gr_row_ok(p, (int)r, &a)) p.moves[r] = 0;
}

// g[:, 64 C ..] += Dl[:, 0 .. 63] * H[64 B .., 64 C ..]: blockIdx.x = C, blockIdx.y = group of 64 rows; wave w takes the
// columns 16 w .. 16 w + 15 of C and every 16-row tile of the group
__global__ __launch_bounds__(256) void k_gr_update(const GrArgs p, const double* __restrict__ Dl, int ld, int B,
                                                   int own) {
  __shared__ float Ts[GQ_B * GR_LDT];      // Ts[c][k] = A0 element that is H[64 B + k][64 C + c]
  if (*p.pd_flag != 0) return;
  const int C = (int)blockIdx.x;
  if (C == B && !own) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const int kb = B * GQ_B, cb = C * GQ_B, n = p.n;
  const int cw = wid * 16 + lr;            // this lane's column inside C
  double bv[GQ_B / 4];
  if (C > B) {                             // the upper triangle as it lies: row 64 B + k, 16 consecutive columns
    const int col = cb + cw;
#pragma unroll
    for (int ks = 0; ks < GQ_B / 4; ++ks) {
      const int row = kb + ks * 4 + lk;
      bv[ks] = (row < n && col < n) ? (double)p.A0[(size_t)row * n + col] : 0.0;
    }
  } else {                                 // the mirror element: rows of A0 along k into LDS, read out along c
    for (int e = tid; e < GQ_B * GQ_B; e += 256) {
      const int c = e >> 6, k = e & 63;
      const int gr = kb + k, gc = cb + c;
      float v = 0.0f;
      if (gr < n && gc < n) v = (gc <= gr) ? p.A0[(size_t)gc * n + gr] : p.A0[(size_t)gr * n + gc];
      Ts[c * GR_LDT + k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < GQ_B / 4; ++ks) {
      const int k = ks * 4 + lk;
      bv[ks] = (double)Ts[cw * GR_LDT + k];
      if (C == B && k == cw && kb + k < n) bv[ks] += p.eta;
    }
  }
  const size_t col = (size_t)cb + cw;
  for (int mi = 0; mi < 4; ++mi) {
    const int row0 = ((int)blockIdx.y * 4 + mi) * 16;
    if (row0 >= p.c2pad) break;
    const double* Dr = Dl + (size_t)(row0 + lr) * ld + lk;
    double* gb = p.g + (size_t)(row0 + lk) * p.npad + col;
    gq_f64x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = gb[(size_t)(4 * r) * p.npad];
#pragma unroll
    for (int ks = 0; ks < GQ_B / 4; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Dr[ks * 4], bv[ks], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) gb[(size_t)(4 * r) * p.npad] = acc[r];
  }
}

// Block B of a pass for the rows 4 blockIdx.x .. + 3: the rule of gptq.py on the columns 64 B .. 64 B + 63
__global__ __launch_bounds__(64 * GQ_ROWS) void k_gr_block(const GrArgs p, int B) {
  __shared__ double Hb[GQ_B * GQ_B];
  if (*p.pd_flag != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int kb = B * GQ_B, n = p.n;
  for (int e = tid; e < GQ_B * GQ_B; e += 64 * GQ_ROWS) {
    const int i = e >> 6, j = e & 63;
    const int gi = kb + i, gj = kb + j;
    double v = (i == j) ? 1.0 : 0.0;       // the padding: never stepped on, feeds nothing
    if (gi < n && gj < n) {
      v = (double)((gi <= gj) ? p.A0[(size_t)gi * n + gj] : p.A0[(size_t)gj * n + gi]);
      if (i == j) v += p.eta;
    }
    Hb[e] = v;
  }
  __syncthreads();
  const int r = (int)blockIdx.x * GQ_ROWS + wid;
  if (r >= p.c2) return;
  double a;
  if (!gr_row_ok(p, r, &a)) return;        // nothing of this row is written; its Delta stays 0 from k_gr_init
  const int col = kb + lane;
  const bool valid = col < n;
  const bool is_bias = p.has_bias && col == n - 1;
  const size_t at = (size_t)r * p.npad + col;
  const double q0 = p.q[at];
  double q = q0, g = p.g[at];
  double idx_mine = (valid && !is_bias) ? (double)p.ids[(size_t)r * p.nw + col] : 0.0;
  const double d = 2.0 / (double)(p.levels - 1);
  bool moved = false;
  const int top = (n - kb < GQ_B) ? n - kb : GQ_B;       // the padding of the last block takes no step
  for (int jj = 0; jj < top; ++jj) {
    const double hjj = Hb[jj * GQ_B + jj];
    const double t = q - g / hjj;                        // every lane computes, lane jj's value is the step's
    double idx = 0.0, qn = t;
    if (!is_bias) qn = a * disc64(t, a, -1.0, 1.0, d, &idx);
    const double en = qn - t, eo = q - t;
    const bool take = is_bias || en * en < eo * eo;
    const double dj = gq_readlane(take ? qn - q : 0.0, jj);
    if (lane == jj && take) {
      q = qn;                                            // the grid value itself
      idx_mine = idx;
      moved = !is_bias;
    }
    if (dj != 0.0) g += dj * Hb[jj * GQ_B + lane];       // (dj is the same in every lane: a uniform branch)
  }
  p.Delta[(size_t)r * GQ_B + lane] = valid ? q - q0 : 0.0;
  if (valid) {
    p.q[at] = q;
    p.g[at] = g;
    if (is_bias) {
      p.b[r] = (float)q;
    } else {
      p.G[(size_t)r * p.nw + col] = gq_weight_f32(a, idx_mine, d, p.per_row);
      p.ids[(size_t)r * p.nw + col] = (uint8_t)idx_mine;
    }
  }
  const int cnt = __popcll(__ballot(moved));
  if (lane == 0) p.moves[r] += cnt;
}

__global__ __launch_bounds__(64 * GQ_ROWS) void k_gr_err(const GrArgs p) {
  if (*p.pd_flag != 0) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = (int)blockIdx.x * GQ_ROWS + wid;
  if (r >= p.c2) return;
  double a;
  if (!gr_row_ok(p, r, &a)) return;
  double s = 0.0;
  for (int c = lane; c < p.n; c += 64) {
    const size_t at = (size_t)r * p.npad + c;
    s += p.g[at] * (p.q[at] - gr_ustar(p, r, c));
  }
  s = wave_sum_f64_dpp(s);                 // (whole waves get here: the returns above are the same in every lane)
  if (lane == 0) p.err[r] = s;
}

}  // namespace effq

using namespace effq;

extern "C" {

size_t effq_gptq_refine_ws_bytes(int c2, int n) {
  if (n < 1 || n > GQ_MAX_N || c2 < 1) return 0;
  const size_t npad = (size_t)round_up(n, GQ_B), c2pad = (size_t)round_up(c2, 16);
  return c2pad * (3 * npad + GQ_B) * sizeof(double) + 256;
}

int effq_gptq_refine_plan_query(int c2, int n, int passes, int* nblk, int* launches, int* block_grid, int* update_gx,
                                int* update_gy) {
  EFFQ_CHECK_ARG(c2 >= 1 && n >= 1 && n <= GQ_MAX_N && passes >= 1 && passes <= GR_MAX_PASSES && nblk && launches &&
                 block_grid && update_gx && update_gy);
  const int nb = round_up(n, GQ_B) / GQ_B;
  *nblk = nb;
  // the initial state and g block by block; per pass a block kernel and, where other blocks exist, their update; the error
  *launches = 1 + nb + passes * (nb > 1 ? 2 * nb : nb) + 1;
  *block_grid = (c2 + GQ_ROWS - 1) / GQ_ROWS;
  *update_gx = nb;
  *update_gy = (round_up(c2, 16) + 63) / 64;
  return EFFQ_OK;
}

int effq_gptq_refine(const float* A0, double eta, int n, const float* uw, const float* ub, int c2, int has_bias,
                     const double* alpha, int per_row, int levels, int passes, float* G, float* b, uint8_t* ids, double* err,
                     int32_t* moves, const int32_t* row_flag, const int* pd_flag, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(A0 && alpha && err && moves && row_flag && pd_flag && ws && n >= 1 && n <= GQ_MAX_N && c2 >= 1);
  EFFQ_CHECK_ARG(eta > 0.0 && eta <= 1.79e308);
  EFFQ_CHECK_ARG(levels >= 2 && levels <= FP_LEVELS_MAX);
  EFFQ_CHECK_ARG(passes >= 1 && passes <= GR_MAX_PASSES);
  const int hb = has_bias ? 1 : 0, nw = n - hb;
  EFFQ_CHECK_ARG(!hb || (ub != nullptr && b != nullptr));
  EFFQ_CHECK_ARG(nw == 0 || (uw != nullptr && G != nullptr && ids != nullptr));
  EFFQ_CHECK_WS(ws_bytes, effq_gptq_refine_ws_bytes(c2, n));
  const int npad = round_up(n, GQ_B), nb = npad / GQ_B, c2pad = round_up(c2, 16);
  GrArgs p;
  p.A0 = A0; p.uw = uw; p.ub = ub; p.alpha = alpha; p.row_flag = row_flag; p.pd_flag = pd_flag;
  p.g = reinterpret_cast<double*>(ws);
  p.q = p.g + (size_t)c2pad * npad;
  p.D = p.q + (size_t)c2pad * npad;
  p.Delta = p.D + (size_t)c2pad * npad;
  p.G = G; p.b = b; p.ids = ids; p.err = err; p.moves = moves; p.eta = eta;
  p.n = n; p.npad = npad; p.nw = nw; p.c2 = c2; p.c2pad = c2pad; p.has_bias = hb; p.per_row = per_row ? 1 : 0;
  p.levels = levels;
  hipStream_t st = as_stream(stream);
  size_t gi = ((size_t)c2pad * npad + 255) / 256;
  if (gi > 4096) gi = 4096;
  const dim3 gu(nb, (c2pad + 63) / 64), gb((c2 + GQ_ROWS - 1) / GQ_ROWS);
  hipLaunchKernelGGL(k_gr_init, dim3((unsigned)gi), dim3(256), 0, st, p);
  EFFQ_LAUNCH_CHECK();
  for (int B = 0; B < nb; ++B)
    hipLaunchKernelGGL(k_gr_update, gu, dim3(256), 0, st, p, (const double*)(p.D + (size_t)B * GQ_B), npad, B, 1);
  EFFQ_LAUNCH_CHECK();
  for (int k = 0; k < passes; ++k)
    for (int B = 0; B < nb; ++B) {
      hipLaunchKernelGGL(k_gr_block, gb, dim3(64 * GQ_ROWS), 0, st, p, B);
      if (nb > 1) hipLaunchKernelGGL(k_gr_update, gu, dim3(256), 0, st, p, (const double*)p.Delta, GQ_B, B, 0);
      EFFQ_LAUNCH_CHECK();
    }
  hipLaunchKernelGGL(k_gr_err, gb, dim3(64 * GQ_ROWS), 0, st, p);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
