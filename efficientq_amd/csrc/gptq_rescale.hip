// The weight scale (and the bias) of every output row refitted on the layer's own quadratic form, the level ids fixed: the
// closed-form minimiser of  f(alpha, beta) = ([alpha v | beta] - u) H ([alpha v | beta] - u)^T,  H = A0 + eta I.  The rule is
// rescale_host of efficientq_amd/gptq.py.  It needs, per row,
//   a11 = v H v^T,  a12 = (v' H)_bias,  c1 = v' H u^T,  c2 = (u H)_bias,  c0 = u H u^T      (v' = [v | 0]),
// i.e. the product of the 2 c2 stacked rows [v' ; u] with the symmetric n x n matrix that exists only as the fp32 upper
// triangle of A0.  Neither the fp64 operands, nor H, nor the product is ever stored:
//   k_gs_forms   one workgroup per run of 64 x 64 tiles (B, C), B <= C, of A0's upper triangle and per group of 32 output
//                rows.  The four waves split the 64 columns of C; a wave converts its 64 x 16 slice of the tile to fp64 in
//                registers once (straight from A0 for B < C; the diagonal tile is mirrored through LDS and takes eta) and
//                keeps it across the row tiles.  The operand slices [v' ; u][:, B] and [:, C] are staged in LDS as the
//                fp32 level ids and the fp32 u; v = id d - 1 is formed in fp64 on the way into the matrix instruction.
//                Per 16-row tile P_v = v'_B T and P_u = u_B T run on v_mfma_f64_16x16x4_f64 and are dotted at once with the
//                slices of C.  The mirrored half H[C, B] = T^T is never multiplied: its contribution to every form is the
//                direct one with the two slices exchanged (v'_C T^T v'_B^T = v'_B T v'_C^T, v'_C T^T u_B^T = u_B T v'_C^T),
//                so an off-diagonal tile counts twice in a11 and c0 and adds P_u . v'_C to c1; one read of A0's triangle
//                and half the product serve the whole matrix.  The bias column is picked from the tiles of the last C.
//                The lanes keep their share of the forms in registers over all tiles of the run; at the end a fixed tree
//                (DPP over the 16 lanes of a row, the four waves in order through LDS) leaves one partial per row and
//                form in the workspace: part[run][row][form].
//   k_gs_reduce  one wave per row adds the runs' partials (lane l takes the runs l, l + 64, ..., then the fixed wave tree),
//                and notes whether the row may be refitted at all (its flag, its present scale).
//   k_gs_solve   one wave per row: the 2 x 2 solve in its Schur form, the guards and `kept`, alpha, b and err, and G rewritten
//                from the ids.  Per tensor every wave adds the rows' numerators and denominators in row order itself.
// No floating-point atomics, nothing is read back.  Every kernel reads the factor's "not positive definite" word first and
// returns when it is set; a flagged row writes nothing.
#include <math.h>
#include "common.h"
#include "fp_level.h"
#include "gptq.h"

namespace effq {

constexpr int GS_ROWS = 32;          // output rows per workgroup of k_gs_forms: two 16-row tiles
constexpr int GS_LD = 68;            // LDS leading dimension (floats) of the operand slices: lane (lr, lk) reads bank 4 lr + lk
constexpr int GS_LDT = 65;           // ... of the diagonal tile that is read out transposed
constexpr int GS_MAX_RUNS = 1024;    // runs of tiles, i.e. partials per row and form
constexpr int GS_FORMS = 5;          // a11, c1, c0, a12, c2
constexpr int GS_ROW_DOUBLES = 8;    // per row after k_gs_reduce: the five forms, then 1.0 where the row may be refitted

struct GsArgs {
  const float *A0, *uw, *ub;         // u*: weights [c2][nw], bias [c2] (or NULL)
  const uint8_t* ids;
  const int32_t* row_flag;
  const int* pd_flag;
  double* part;                      // [runs][c2pad][GS_FORMS]
  double* rows;                      // [c2][GS_ROW_DOUBLES]
  double* alpha;
  float *G, *b;
  double* err;
  int32_t* kept;
  double eta;
  int n, nw, c2, c2pad, has_bias, per_row, levels, ntiles, tiles_per_run, runs;
};

static inline int gs_tiles(int n) {
  const int nb = round_up(n, GQ_B) / GQ_B;
  return nb * (nb + 1) / 2;
}
static inline int gs_tiles_per_run(int n) { return (gs_tiles(n) + GS_MAX_RUNS - 1) / GS_MAX_RUNS; }
static inline int gs_runs(int n) { return (gs_tiles(n) + gs_tiles_per_run(n) - 1) / gs_tiles_per_run(n); }

// the level value of a staged id; the padding, the bias column and rows past c2 are staged as -1 and give 0
__device__ __forceinline__ double gs_level(float idf, double d) { return idf >= 0.0f ? (double)idf * d + -1.0 : 0.0; }

// the sum over the 16 lanes of a DPP row, in every lane of it (all 64 lanes are active at every call site)
__device__ __forceinline__ double gs_row16_sum(double v) {
  v += dpp_f64<DPP_XOR1>(v);
  v += dpp_f64<DPP_XOR2>(v);
  v += dpp_f64<DPP_HALF_MIRROR>(v);
  v += dpp_f64<DPP_MIRROR>(v);
  return v;
}

__global__ __launch_bounds__(256) void k_gs_forms(const GsArgs p) {
  __shared__ float Xs[2][2][GS_ROWS * GS_LD];      // [block B, block C][level id, u][row][column]
  __shared__ float Ts[GQ_B * GS_LDT];              // the diagonal tile: Ts[c][k] = H[64 B + k][64 B + c] without eta
  __shared__ double Rs[4][GS_ROWS][GS_FORMS];
  if (*p.pd_flag != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const int groups = p.c2pad / GS_ROWS;
  const int grp = (int)blockIdx.x % groups, run = (int)blockIdx.x / groups;   // the groups of a run side by side: one tile in cache
  const int row0 = grp * GS_ROWS, n = p.n;
  const int cw = wid * 16 + lr;                    // this lane's column inside C
  const double d = 2.0 / (double)(p.levels - 1);
  const int bias_col = p.has_bias ? n - 1 : -1;
  double f[2][4][GS_FORMS];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s < GS_FORMS; ++s) f[mi][r][s] = 0.0;
  const int t1 = min(p.ntiles, (run + 1) * p.tiles_per_run);
  for (int t = run * p.tiles_per_run; t < t1; ++t) {
    int C = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);               // tiles in the order (0,0) (0,1) (1,1) (0,2) ...
    while (C * (C + 1) / 2 > t) --C;
    while ((C + 1) * (C + 2) / 2 <= t) ++C;
    const int B = t - C * (C + 1) / 2;
    const int kb = B * GQ_B, cb = C * GQ_B;
    const bool diag = B == C;
    __syncthreads();                               // the previous tile's readers are done with Xs and Ts
    for (int side = 0; side < (diag ? 1 : 2); ++side) {
      const int base = side ? cb : kb;
      for (int e = tid; e < GS_ROWS * GQ_B; e += 256) {
        const int r = e >> 6, c = e & 63;
        const int gr = row0 + r, gc = base + c;
        float idf = -1.0f, uf = 0.0f;
        if (gr < p.c2 && gc < n) {
          if (gc == bias_col) {
            uf = p.ub[gr];
          } else {
            idf = (float)p.ids[(size_t)gr * p.nw + gc];
            uf = p.uw[(size_t)gr * p.nw + gc];
          }
        }
        Xs[side][0][r * GS_LD + c] = idf;
        Xs[side][1][r * GS_LD + c] = uf;
      }
    }
    double bv[GQ_B / 4];                           // H[64 B + 4 ks + lk][64 C + cw]
    if (!diag) {                                   // the upper triangle as it lies: 16 consecutive floats per row and wave
      const int col = cb + cw;
#pragma unroll
      for (int ks = 0; ks < GQ_B / 4; ++ks) {
        const int row = kb + ks * 4 + lk;
        bv[ks] = (row < n && col < n) ? (double)p.A0[(size_t)row * n + col] : 0.0;
      }
      __syncthreads();
    } else {
      for (int e = tid; e < GQ_B * GQ_B; e += 256) {
        const int k = e >> 6, c = e & 63;          // coalesced along c; the element of the upper triangle serves both
        const int gr = kb + k, gc = kb + c;
        float v = 0.0f;
        if (gr < n && gc < n) v = (gr <= gc) ? p.A0[(size_t)gr * n + gc] : p.A0[(size_t)gc * n + gr];
        Ts[c * GS_LDT + k] = v;
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < GQ_B / 4; ++ks) {
        const int k = ks * 4 + lk;
        bv[ks] = (double)Ts[cw * GS_LDT + k];
        if (k == cw && kb + k < n) bv[ks] += p.eta;
      }
    }
    const float* XB = Xs[0][0];
    const float* XC = Xs[diag ? 0 : 1][0];
    const double twice = diag ? 1.0 : 2.0;
    const bool pick = bias_col >= 0 && cb + cw == bias_col;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const float* ar = XB + (mi * 16 + lr) * GS_LD + lk;
      gq_f64x4 pv = {0.0, 0.0, 0.0, 0.0}, pu = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < GQ_B / 4; ++ks) {
        const double av = gs_level(ar[ks * 4], d), au = (double)ar[GS_ROWS * GS_LD + ks * 4];
        pv = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[ks], pv, 0, 0, 0);
        pu = __builtin_amdgcn_mfma_f64_16x16x4f64(au, bv[ks], pu, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {                // the product's element (row 16 mi + lk + 4 r, column cw)
        const float* cr = XC + (mi * 16 + lk + 4 * r) * GS_LD + cw;
        const double vc = gs_level(cr[0], d), uc = (double)cr[GS_ROWS * GS_LD];
        f[mi][r][0] += twice * (pv[r] * vc);
        f[mi][r][1] += pv[r] * uc;
        if (!diag) f[mi][r][1] += pu[r] * vc;
        f[mi][r][2] += twice * (pu[r] * uc);
        if (pick) {
          f[mi][r][3] += pv[r];
          f[mi][r][4] += pu[r];
        }
      }
    }
  }
  // one partial per row and form: the 16 lanes of a DPP row, then the four waves in order
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s < GS_FORMS; ++s) {
        const double v = gs_row16_sum(f[mi][r][s]);
        if (lr == 0) Rs[wid][mi * 16 + lk + 4 * r][s] = v;
      }
  __syncthreads();
  if (tid < GS_ROWS * GS_FORMS) {
    const int r = tid / GS_FORMS, s = tid % GS_FORMS;
    p.part[((size_t)run * p.c2pad + row0 + r) * GS_FORMS + s] = ((Rs[0][r][s] + Rs[1][r][s]) + Rs[2][r][s]) + Rs[3][r][s];
  }
}

__global__ __launch_bounds__(64 * GQ_ROWS) void k_gs_reduce(const GsArgs p) {
  if (*p.pd_flag != 0) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = (int)blockIdx.x * GQ_ROWS + wid;
  if (r >= p.c2) return;                           // (whole waves: the tree below needs every lane)
  double s[GS_FORMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int run = lane; run < p.runs; run += 64) {
    const double* pr = p.part + ((size_t)run * p.c2pad + r) * GS_FORMS;
#pragma unroll
    for (int k = 0; k < GS_FORMS; ++k) s[k] += pr[k];
  }
#pragma unroll
  for (int k = 0; k < GS_FORMS; ++k) s[k] = wave_sum_f64_dpp(s[k]);
  if (lane == 0) {
    double* out = p.rows + (size_t)r * GS_ROW_DOUBLES;
#pragma unroll
    for (int k = 0; k < GS_FORMS; ++k) out[k] = s[k];
    const double a = p.alpha[p.per_row ? r : 0];
    out[GS_FORMS] = (p.row_flag[r] == 0 && a > 0.0 && a <= 1.79e308) ? 1.0 : 0.0;
  }
}

// numerator and denominator of the scale with the bias eliminated (the Schur complement of a22)
__device__ __forceinline__ void gs_num_den(const double* row, double a22, int has_bias, double* num, double* den) {
  *num = has_bias ? row[1] - row[3] * row[4] / a22 : row[1];
  *den = has_bias ? row[0] - row[3] * row[3] / a22 : row[0];
}

__global__ __launch_bounds__(64 * GQ_ROWS) void k_gs_solve(const GsArgs p) {
  if (*p.pd_flag != 0) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = (int)blockIdx.x * GQ_ROWS + wid;
  if (r >= p.c2) return;
  const int n = p.n;
  const double* row = p.rows + (size_t)r * GS_ROW_DOUBLES;
  if (row[GS_FORMS] == 0.0) {                      // a flagged row writes nothing
    if (p.per_row && lane == 0) atomicAdd(p.kept, 1);
    if (!p.per_row && r == 0 && lane == 0) atomicAdd(p.kept, 1);
    return;
  }
  const double a22 = p.has_bias ? (double)p.A0[(size_t)(n - 1) * n + (n - 1)] + p.eta : 1.0;
  double num, den;
  bool ok = true;
  if (p.per_row) {
    gs_num_den(row, a22, p.has_bias, &num, &den);
  } else {                                         // every wave adds the rows in row order: the same sums everywhere
    num = 0.0;
    den = 0.0;
    for (int i = 0; i < p.c2; ++i) {
      const double* ri = p.rows + (size_t)i * GS_ROW_DOUBLES;
      double ni, di;
      gs_num_den(ri, a22, p.has_bias, &ni, &di);
      num += ni;
      den += di;
      ok = ok && ri[GS_FORMS] != 0.0;
    }
  }
  double a = num / den;
  double beta = p.has_bias ? (row[4] - row[3] * a) / a22 : 0.0;
  ok = ok && den > 0.0 && a > 0.0 && a <= 1.79e308 && fabs(beta) <= 1.79e308;
  if (!p.per_row && p.has_bias)                    // one scale: it is taken by every row or by none
    for (int i = 0; i < p.c2; ++i) {
      const double* ri = p.rows + (size_t)i * GS_ROW_DOUBLES;
      ok = ok && fabs((ri[4] - ri[3] * a) / a22) <= 1.79e308;
    }
  const bool taken = ok;
  if (!taken) {                                    // the point the row stands on
    a = p.alpha[p.per_row ? r : 0];
    beta = p.has_bias ? (double)p.b[r] : 0.0;
    if (lane == 0 && (p.per_row || r == 0)) atomicAdd(p.kept, 1);
  }
  if (lane == 0)
    p.err[r] = a * a * row[0] + 2.0 * a * beta * row[3] + beta * beta * (p.has_bias ? a22 : 0.0) - 2.0 * a * row[1] -
               2.0 * beta * row[4] + row[2];
  if (!taken) return;
  if (lane == 0) {
    if (p.per_row || r == 0) p.alpha[p.per_row ? r : 0] = a;
    if (p.has_bias) p.b[r] = (float)beta;
  }
  const double d = 2.0 / (double)(p.levels - 1);
  for (int c = lane; c < p.nw; c += 64) {
    const size_t at = (size_t)r * p.nw + c;
    p.G[at] = gq_weight_f32(a, (double)p.ids[at], d, p.per_row);
  }
}

}  // namespace effq

using namespace effq;

extern "C" {

size_t effq_gptq_rescale_ws_bytes(int c2, int n) {
  if (n < 1 || n > GQ_MAX_N || c2 < 1) return 0;
  const size_t c2pad = (size_t)round_up(c2, GS_ROWS);
  return ((size_t)gs_runs(n) * c2pad * GS_FORMS + (size_t)c2 * GS_ROW_DOUBLES) * sizeof(double) + 256;
}

int effq_gptq_rescale_plan_query(int c2, int n, int* nblk, int* tiles, int* tiles_per_run, int* runs, int* forms_grid,
                                 int* launches) {
  EFFQ_CHECK_ARG(c2 >= 1 && n >= 1 && n <= GQ_MAX_N && nblk && tiles && tiles_per_run && runs && forms_grid && launches);
  *nblk = round_up(n, GQ_B) / GQ_B;
  *tiles = gs_tiles(n);
  *tiles_per_run = gs_tiles_per_run(n);
  *runs = gs_runs(n);
  *forms_grid = gs_runs(n) * (round_up(c2, GS_ROWS) / GS_ROWS);
  *launches = 3;
  return EFFQ_OK;
}

int effq_gptq_rescale(const float* A0, double eta, int n, const float* uw, const float* ub, int c2, int has_bias,
                      const uint8_t* ids, int levels, int per_row, const int32_t* row_flag, const int* pd_flag,
                      double* alpha, float* G, float* b, double* err, int32_t* kept, void* ws, size_t ws_bytes,
                      void* stream) {
  EFFQ_CHECK_ARG(A0 && alpha && err && kept && row_flag && pd_flag && ws && n >= 1 && n <= GQ_MAX_N && c2 >= 1);
  EFFQ_CHECK_ARG(eta > 0.0 && eta <= 1.79e308);
  EFFQ_CHECK_ARG(levels >= 2 && levels <= FP_LEVELS_MAX);
  const int hb = has_bias ? 1 : 0, nw = n - hb;
  EFFQ_CHECK_ARG(!hb || (ub != nullptr && b != nullptr));
  EFFQ_CHECK_ARG(nw == 0 || (uw != nullptr && G != nullptr && ids != nullptr));
  EFFQ_CHECK_WS(ws_bytes, effq_gptq_rescale_ws_bytes(c2, n));
  GsArgs p;
  p.A0 = A0; p.uw = uw; p.ub = ub; p.ids = ids; p.row_flag = row_flag; p.pd_flag = pd_flag;
  p.c2 = c2; p.c2pad = round_up(c2, GS_ROWS); p.n = n; p.nw = nw; p.has_bias = hb; p.per_row = per_row ? 1 : 0;
  p.levels = levels; p.ntiles = gs_tiles(n); p.tiles_per_run = gs_tiles_per_run(n); p.runs = gs_runs(n);
  p.part = reinterpret_cast<double*>(ws);
  p.rows = p.part + (size_t)p.runs * p.c2pad * GS_FORMS;
  p.alpha = alpha; p.G = G; p.b = b; p.err = err; p.kept = kept; p.eta = eta;
  hipStream_t st = as_stream(stream);
  const dim3 gf((unsigned)(p.runs * (p.c2pad / GS_ROWS))), gr((c2 + GQ_ROWS - 1) / GQ_ROWS);
  hipLaunchKernelGGL(k_gs_forms, gf, dim3(256), 0, st, p);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gs_reduce, gr, dim3(64 * GQ_ROWS), 0, st, p);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gs_solve, gr, dim3(64 * GQ_ROWS), 0, st, p);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
