// Proximal step of the ADMM, first half: the system matrix and its fp64 SPD inverse (cached per rho by the caller).
// The per-iteration product  What = B * A^-1  is prox_solve.hip.
// Reference: solver.py:316-325 (getAB), :327-345 (solve; torch.linalg.solve = LU, every iteration).
//
// A = A0 + rho*I' + eta*I is symmetric positive definite (PSD Gram + eta*I, eta>0), and it changes
// only when rho does (5 values per layer), so the inverse is formed once per rho in fp64 by a
// blocked in-place Gauss-Jordan sweep (no pivoting needed for SPD) whose bulk is a rank-64 fp64
// MFMA update (v_mfma_f64_16x16x4_f64), then rounded once to fp32.
#include <vector>
#include "common.h"

namespace effq {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int NBK = 64;        // Gauss-Jordan block size
constexpr int LDA_S = 66;      // LDS leading dims (doubles): conflict-free ds_read_b64 operand fetches
constexpr int LDB_S = 80;

// A64 (npad x npad, row-major) = A0 + diag, identity on the padding
__global__ __launch_bounds__(256) void k_build_a64(const float* __restrict__ A0, int n, int npad, int has_bias,
                                                   double rho, double eta, double* __restrict__ A64) {
  const size_t tot = (size_t)npad * npad;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += stride) {
    const int i = (int)(e / npad), j = (int)(e % npad);
    double v = 0.0;
    if (i < n && j < n) {
      v = (double)A0[(size_t)i * n + j];
      if (i == j) v += eta + ((has_bias && i == n - 1) ? 0.0 : rho);
    } else if (i == j) {
      v = 1.0;
    }
    A64[e] = v;
  }
}

// Step 1: Dinv = inv(A[kb:kb+64, kb:kb+64]) by unblocked in-place Gauss-Jordan (SPD: no pivoting).
// Lane = row, wave w = columns 16w..16w+15, the 16 values of a row live in registers.  Per pivot p the
// multiplier column and 1/pivot go through a parity-double-buffered LDS vector (ONE barrier per
// pivot), the pivot row is broadcast inside each wave with v_readlane.
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// In-register Gauss-Jordan inverse of a 64 x 64 block held as lane = row, wave w = columns CPW w .. CPW w + CPW - 1
// (64 / CPW waves take part).  fcol: [2][NBK + 1] doubles of LDS.
template <int CPW>
__device__ __forceinline__ void gj_invert_regs(double (&reg)[CPW], double (*fcol)[NBK + 1], int lane, int wid) {
#pragma unroll
  for (int p = 0; p < NBK; ++p) {      // fully unrolled: pivot column / lane selectors become immediates
    const int par = p & 1, wp = p / CPW, jp = p % CPW;
    if (wid == wp) {
      double cp = reg[0];
#pragma unroll
      for (int j = 1; j < CPW; ++j) cp = (jp == j) ? reg[j] : cp;
      fcol[par][lane] = cp;
      if (lane == p) fcol[par][NBK] = 1.0 / cp;
    }
    lds_barrier();
    const double piv = fcol[par][NBK];
    const double f = fcol[par][lane];
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
      const double rp = readlane_f64(reg[j], p) * piv;      // scaled pivot-row entry of this column
      const bool colp = (wid == wp) && (jp == j);
      double v;
      if (lane == p)
        v = colp ? piv : rp;
      else
        v = colp ? (-f * piv) : (reg[j] - f * rp);
      reg[j] = v;
    }
  }
}

// 16 waves, 4 columns of the 64 x 64 block per wave (lane = row): a pivot step costs every wave 4 column updates
// (the 4-wave version, 16 columns per wave, took 32 us per block - 64 serial steps of ~1500 cycles - on the critical
// path of every inverse).  Only the FIRST pivot block of an inverse is inverted by this kernel: the later ones are
// inverted by a workgroup of the preceding trailing update (k_gj_trail_sym), under that update.
constexpr int GJD_T = 1024, GJD_CPW = NBK / (GJD_T / 64);     // columns per wave = 4
__global__ __launch_bounds__(GJD_T) void k_gj_diag(const double* __restrict__ A, int npad, int kb,
                                                   double* __restrict__ Dinv) {
  __shared__ double fcol[2][NBK + 1];   // [parity][row] multipliers, [NBK] = 1/pivot
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  double reg[GJD_CPW];
#pragma unroll
  for (int j = 0; j < GJD_CPW; ++j) reg[j] = A[(size_t)(kb + lane) * npad + kb + wid * GJD_CPW + j];
  gj_invert_regs<GJD_CPW>(reg, fcol, lane, wid);
#pragma unroll
  for (int j = 0; j < GJD_CPW; ++j) Dinv[lane * NBK + wid * GJD_CPW + j] = reg[j];
}

// 64x64x64 fp64 tile product on the matrix cores: acc += As(64x64) * Bs(64x64), one 32x32 quadrant per wave.
__device__ __forceinline__ void tile_mma64(const double* As, const double* Bs, f64x4 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll 4
  for (int ks = 0; ks < NBK / 4; ++ks) {
    double a[2], b[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) a[mi] = As[(wr * 32 + mi * 16 + lr) * LDA_S + ks * 4 + lk];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) b[ni] = Bs[(ks * 4 + lk) * LDB_S + wc * 32 + ni * 16 + lr];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
  }
}

// (The accumulator-tile loops and the global-B MFMA strip of k_gj_panel, k_gj_trail_sym and k_gj_panel_w stay written
// out in each kernel: composed of shared helpers the kernels missed their registers or their time, see
// profiles/solve_split_ab.txt.)
__device__ __forceinline__ void load_tile(double* dst, int ld, const double* src, size_t src_ld) {
  // 64x64 doubles, 256 threads, 16 per thread, coalesced along rows
  const int tid = threadIdx.x;
  for (int e = tid; e < NBK * NBK; e += 256) {
    const int r = e >> 6, c = e & 63;
    dst[r * ld + c] = src[(size_t)r * src_ld + c];
  }
}

constexpr int GJ_CT = 4;     // column blocks per workgroup of the trailing update

// ---- symmetric block Gauss-Jordan ---------------------------------------------------------------------
// A is symmetric, and block Gauss-Jordan keeps a signed symmetry: with S = the pivot blocks already processed
// and U the rest, M_ji = M_ij^T when i, j are both in S or both in U, and M_ji = -M_ij^T otherwise.  Only the
// UPPER block triangle is therefore stored and updated: half the flops and - what matters, the rank-64 update
// is HBM-bound - half the bytes per elimination step.  Per pivot block k:
//   X_t = M_tk for every block row t != k   (t < k: block (t,k);  t > k: block (k,t)^T)
//   Z_t = X_t * Dinv                        (Dinv = inv(M_kk), k_gj_diag)
//   M_ij -= Z_i * (s_j X_j^T)  for i <= j, i, j != k,  s_j = -1 for j < k (j in S, k in U), +1 for j > k
//   new M_tk = -Z_t (t < k),  new M_kt = Z_t^T (t > k),  new M_kk = Dinv.
// k_gj_panel forms NZ = -Z (npad x 64, the A operand of the update) and XT = s * X^T (64 x npad, the B operand
// in MFMA layout, coalesced) and writes the new pivot row/column; k_gj_trail_sym is the old trailing update on
// the upper triangle with those operands.
__global__ __launch_bounds__(256) void k_gj_panel(double* __restrict__ A, int npad, int kb,
                                                  const double* __restrict__ Dinv, double* __restrict__ NZ,
                                                  double* __restrict__ XT) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* As = sm;                  // X_t  [64][LDA_S]
  double* Bs = sm + NBK * LDA_S;    // Dinv [64][LDB_S]
  const int kblk = kb / NBK;
  const int t = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  if (t == kblk) {                  // A[kb,kb] = Dinv
    for (int e = tid; e < NBK * NBK; e += 256) A[(size_t)(kb + (e >> 6)) * npad + kb + (e & 63)] = Dinv[e];
    return;
  }
  const bool upper = t < kblk;      // X_t is the stored block (t,k); otherwise the transpose of block (k,t)
  const double sgn = upper ? -1.0 : 1.0;
  for (int e = tid; e < NBK * NBK; e += 256) {
    const int r = e >> 6, c = e & 63;
    // stored element (r,c) of the source block; for the transposed case it is X[c][r]
    const double v = upper ? A[(size_t)(t * NBK + r) * npad + kb + c] : A[(size_t)(kb + r) * npad + (size_t)t * NBK + c];
    if (upper) {
      As[r * LDA_S + c] = v;                                        // X[r][c]
    } else {
      As[c * LDA_S + r] = v;                                        // X[c][r] = block(k,t)[r][c]
    }
  }
  load_tile(Bs, LDB_S, Dinv, NBK);
  lds_barrier();
  // XT[kk][t*64 + r] = s * X[r][kk]   (coalesced along r)
  for (int e = tid; e < NBK * NBK; e += 256) {
    const int kk = e >> 6, r = e & 63;
    XT[(size_t)kk * npad + (size_t)t * NBK + r] = sgn * As[r * LDA_S + kk];
  }
  f64x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[mi][ni][r] = 0.0;
  tile_mma64(As, Bs, acc);          // Z = X * Dinv
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wr * 32 + mi * 16 + lk + 4 * r;
        const int col = wc * 32 + ni * 16 + lr;
        const double z = acc[mi][ni][r];
        NZ[(size_t)(t * NBK + row) * NBK + col] = -z;
        if (upper)
          A[(size_t)(t * NBK + row) * npad + kb + col] = -z;          // new M_tk
        else
          A[(size_t)(kb + col) * npad + (size_t)t * NBK + row] = z;   // new M_kt = Z^T
      }
}

// blockIdx.y = 0 is the LOOK-AHEAD row: its first workgroup forms the pivot block of the NEXT step - tile (k+1, k+1)
// after this step's update, which it computes itself from the not yet updated tile (the regular workgroups leave that
// tile alone: k_gj_panel of the next step overwrites it with its inverse anyway) - and inverts it in registers, while the
// other workgroups update the rest of the triangle.  The 64 serial pivots (~30 us with 4 waves) that used to sit
// between two trailing updates as a kernel of their own (k_gj_diag: 24 us + a launch gap per 64 columns) are hidden
// under the update.  blockIdx.y = ib + 1 for the regular rows.
__global__ __launch_bounds__(256) void k_gj_trail_sym(double* __restrict__ A, int npad, int kb,
                                                      const double* __restrict__ NZ, const double* __restrict__ XT,
                                                      double* __restrict__ Dinv_next) {
  __shared__ __attribute__((aligned(16))) double As[NBK * LDA_S];
  __shared__ double fcol[2][NBK + 1];
  const int kblk = kb / NBK, nblk = npad / NBK;
  const int kn = kblk + 1;                                         // the next pivot block
  const bool ahead = Dinv_next != nullptr && kn < nblk;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int lr = lane & 15, lk = lane >> 4;
  if (blockIdx.y == 0) {
    if (blockIdx.x != 0 || !ahead) return;
    for (int e = tid; e < NBK * NBK; e += 256) {
      const int r = e >> 6, c = e & 63;
      As[r * LDA_S + c] = NZ[(size_t)(kn * NBK + r) * NBK + c];      // -Z_kn
    }
    lds_barrier();
    const double* Cb = A + (size_t)(kn * NBK + wr * 32) * npad + (size_t)kn * NBK + wc * 32;
    const double* Rb = XT + (size_t)kn * NBK + wc * 32;
    f64x4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mi][ni][r] = Cb[(size_t)(mi * 16 + lk + 4 * r) * npad + ni * 16 + lr];
#pragma unroll 4
    for (int ks = 0; ks < NBK / 4; ++ks) {
      double a[2], b[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) a[mi] = As[(wr * 32 + mi * 16 + lr) * LDA_S + ks * 4 + lk];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) b[ni] = Rb[(size_t)(ks * 4 + lk) * npad + ni * 16 + lr];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
    lds_barrier();                                                 // As (the A operand) has been consumed
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          As[(wr * 32 + mi * 16 + lk + 4 * r) * LDA_S + wc * 32 + ni * 16 + lr] = acc[mi][ni][r];
    lds_barrier();
    constexpr int CPW = NBK / 4;                                   // 4 waves, 16 columns each, lane = row
    double reg[CPW];
#pragma unroll
    for (int j = 0; j < CPW; ++j) reg[j] = As[lane * LDA_S + wid * CPW + j];
    gj_invert_regs<CPW>(reg, fcol, lane, wid);
#pragma unroll
    for (int j = 0; j < CPW; ++j) Dinv_next[lane * NBK + wid * CPW + j] = reg[j];
    return;
  }
  const int ib = (int)blockIdx.y - 1;
  if (ib == kblk) return;
  if ((int)(blockIdx.x * GJ_CT + GJ_CT - 1) < ib) return;        // the whole strip lies below the diagonal
  for (int e = tid; e < NBK * NBK; e += 256) {
    const int r = e >> 6, c = e & 63;
    As[r * LDA_S + c] = NZ[(size_t)(ib * NBK + r) * NBK + c];      // -Z_i
  }
  lds_barrier();
  // The strip's tiles in turn, the C tile of the NEXT one fetched into a second register set before the MFMAs of the
  // current one (the update moves 64 KB per 0.5 MFLOP tile: it is bound by memory latency, not by the matrix cores)
  auto live = [&](int t) -> bool {
    const int jb = blockIdx.x * GJ_CT + t;
    return t < GJ_CT && jb < nblk && jb != kblk && jb >= ib && !(ahead && ib == kn && jb == kn);
  };
  auto fetch = [&](int t, f64x4 (&c)[2][2]) {
    const int jb = blockIdx.x * GJ_CT + t;
    const double* Cb = A + (size_t)(ib * NBK + wr * 32) * npad + (size_t)jb * NBK + wc * 32;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) c[mi][ni][r] = Cb[(size_t)(mi * 16 + lk + 4 * r) * npad + ni * 16 + lr];
  };
  f64x4 nxt[2][2];
  int t = 0;
  while (t < GJ_CT && !live(t)) ++t;
  if (t < GJ_CT) fetch(t, nxt);
  while (t < GJ_CT) {
    const int jb = blockIdx.x * GJ_CT + t;
    f64x4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = nxt[mi][ni];
    int tn = t + 1;
    while (tn < GJ_CT && !live(tn)) ++tn;
    if (tn < GJ_CT) fetch(tn, nxt);
    double* Cb = A + (size_t)(ib * NBK + wr * 32) * npad + (size_t)jb * NBK + wc * 32;
    const double* Rb = XT + (size_t)jb * NBK + wc * 32;
#pragma unroll 4
    for (int ks = 0; ks < NBK / 4; ++ks) {
      double a[2], b[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) a[mi] = As[(wr * 32 + mi * 16 + lr) * LDA_S + ks * 4 + lk];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) b[ni] = Rb[(size_t)(ks * 4 + lk) * npad + ni * 16 + lr];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) Cb[(size_t)(mi * 16 + lk + 4 * r) * npad + ni * 16 + lr] = acc[mi][ni][r];
    t = tn;
  }
}

__global__ __launch_bounds__(256) void k_a64_to_f32(const double* __restrict__ A64, int n, int npad,
                                                    float* __restrict__ Ainv, int lda) {
  const size_t tot = (size_t)n * lda;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += stride) {
    const int i = (int)(e / lda), j = (int)(e % lda);
    // only the upper block triangle is maintained (symmetric Gauss-Jordan): mirror it.  Columns >= n are padding.
    const int a = (i < j) ? i : j, b = (i < j) ? j : i;
    Ainv[e] = (j < n) ? (float)A64[(size_t)a * npad + b] : 0.0f;
  }
}

// ======================================================================================================================
// The same symmetric block Gauss-Jordan with pivot blocks of 256 rows (WB = 4 of the 64-blocks above).
//
// The rank-64 sweep reads and writes the stored triangle once per 64 columns: 8 flop per byte moved, an HBM / Infinity-
// Cache stream that left the fp64 matrix cores at a third of their rate (n = 6913: 12.9 ms alone, 27 - 33 ms beside the
// ADMM chain).  With a 256-row pivot block P the elimination step is the same algebra on bigger blocks,
//   X_t = M_tP (t outside P),  Z_t = X_t inv(M_PP),  M_ij -= Z_i (s_j X_j^T),  new M_tP = -+Z_t,  new M_PP = inv(M_PP),
// and the update of the triangle is a rank-256 product: 32 flop per byte of C, four times fewer passes over the matrix.
// Per pivot block:
//   k_gj_panel_w   Z = X inv(M_PP) for every 64-row block outside P -> the operands of the update, both K-major
//                  (NZT = -Z^T, XTW = s X^T: [256][ldx]), nothing written to the matrix yet (the workgroups of one block
//                  row read each other's blocks);
//   k_gj_wback_w   the new pivot rows / columns and inv(M_PP) into the matrix;
//   k_gj_big       the update, 128 x 128 tiles of the upper triangle, K = 256 staged through LDS in chunks of 16;
//   the NEXT pivot block: k_gj_big on its own 256 x 256 tile alone (out of place, into the scratch matrix D), the rank-64
//                  sweep above on D (a 256 x 256 matrix of its own), k_mirror_blocks.  None of that depends on the big
//                  update, which leaves that tile alone: it runs on a helper stream BESIDE the big update, so the serial
//                  pivot work (4 x 64 dependent pivots per pivot block) is off the critical path for n >= ~5000.
constexpr int WB = 4, WK = WB * NBK;
constexpr int BG_T = 128, BG_KC = 16, BG_LD = 144;      // macro tile, K chunk, LDS row pitch (doubles): see the bank notes below
typedef double f64x2 __attribute__((ext_vector_type(2)));

struct GjBig {
  const double* Cin;      // the matrix, addressed in place: block (i, j) at Cin[(i*64)*ldin + j*64]
  size_t ldin;
  double* Cout;           // output: Cout[(i*64 - orow)*ldout + (j*64 - ocol)]  (Cin itself for the in-place update)
  size_t ldout;
  int orow, ocol;
  const double* NZT;      // [kdim][ldx]: -Z^T  (A operand, K-major)
  const double* XTW;      // [kdim][ldx]: s X^T (B operand)
  size_t ldx;
  int kdim;               // 64 * (64-blocks of the pivot); 0 = plain copy
  int nblk;               // 64-blocks per side
  int i0m, j0m;           // macro-tile offset of the grid
  int skip_lo, skip_hi;   // 64-blocks of the pivot: rows / columns left alone
  int la_lo, la_hi;       // 64-blocks of the NEXT pivot: blocks with BOTH indices inside are left alone
};

// One 128 x 128 macro tile per workgroup, one 64 x 64 block per wave (16 accumulator tiles of 16 x 16), K in chunks of 16
// through a double-buffered LDS stage: global -> registers (issued before the MFMAs of the current chunk) -> LDS, one
// barrier per chunk.  Both operands are K-major ([k][row]): an operand fetch is one ds_read_b64 per lane, lanes 0-15 /
// 16-31 of a half-wave read rows k and k+1, 144 doubles = 32 banks (mod 64) apart: conflict-free; the staging stores
// are ds_write_b128 with the 8 lanes of a group 16 B apart.  64 MFMAs (64 cycles each) per wave and chunk against 32
// operand reads and 4 + 4 staging stores: the kernel is paced by the matrix pipe, and by its C traffic (16 B per 512 flop).
__global__ __launch_bounds__(256, 2) void k_gj_big(const GjBig p) {
  __shared__ __attribute__((aligned(16))) double As[2][BG_KC * BG_LD];
  __shared__ __attribute__((aligned(16))) double Bs[2][BG_KC * BG_LD];
  const int I = p.i0m + (int)blockIdx.y, J = p.j0m + (int)blockIdx.x;
  if (J < I) return;
  auto blk_live = [&](int bi, int bj) -> bool {
    if (bi > bj || bj >= p.nblk) return false;
    if ((bi >= p.skip_lo && bi < p.skip_hi) || (bj >= p.skip_lo && bj < p.skip_hi)) return false;
    if (bi >= p.la_lo && bi < p.la_hi && bj >= p.la_lo && bj < p.la_hi) return false;
    return true;
  };
  if (!(blk_live(2 * I, 2 * J) || blk_live(2 * I, 2 * J + 1) || blk_live(2 * I + 1, 2 * J) || blk_live(2 * I + 1, 2 * J + 1)))
    return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int lr = lane & 15, lk = lane >> 4;
  const int bi = 2 * I + wr, bj = 2 * J + wc;
  const bool live = blk_live(bi, bj);
  f64x4 acc[4][4];
  if (live) {
    const double* Cb = p.Cin + (size_t)bi * NBK * p.ldin + (size_t)bj * NBK;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mi][ni][r] = Cb[(size_t)(mi * 16 + lk + 4 * r) * p.ldin + ni * 16 + lr];
  } else {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mi][ni][r] = 0.0;
  }
  const int nch = p.kdim / BG_KC;
  if (nch > 0) {
    const int sk = tid >> 4, sc = (tid & 15) * 2;       // staging: K row, first column (doubles) of the 4 pieces 32 apart
    const double* Ag = p.NZT + (size_t)sk * p.ldx + (size_t)I * BG_T + sc;
    const double* Bg = p.XTW + (size_t)sk * p.ldx + (size_t)J * BG_T + sc;
    f64x2 ra[4], rb[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      ra[v] = *reinterpret_cast<const f64x2*>(Ag + v * 32);
      rb[v] = *reinterpret_cast<const f64x2*>(Bg + v * 32);
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      *reinterpret_cast<f64x2*>(&As[0][sk * BG_LD + sc + v * 32]) = ra[v];
      *reinterpret_cast<f64x2*>(&Bs[0][sk * BG_LD + sc + v * 32]) = rb[v];
    }
    lds_barrier();
    for (int c = 0; c < nch; ++c) {
      const int buf = c & 1;
      if (c + 1 < nch) {
        const size_t off = (size_t)(c + 1) * BG_KC * p.ldx;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          ra[v] = *reinterpret_cast<const f64x2*>(Ag + off + v * 32);
          rb[v] = *reinterpret_cast<const f64x2*>(Bg + off + v * 32);
        }
      }
      if (live) {
#pragma unroll
        for (int ks = 0; ks < BG_KC / 4; ++ks) {
          double a[4], b[4];
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) a[mi] = As[buf][(ks * 4 + lk) * BG_LD + wr * 64 + mi * 16 + lr];
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) b[ni] = Bs[buf][(ks * 4 + lk) * BG_LD + wc * 64 + ni * 16 + lr];
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
        }
      }
      if (c + 1 < nch) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          *reinterpret_cast<f64x2*>(&As[buf ^ 1][sk * BG_LD + sc + v * 32]) = ra[v];
          *reinterpret_cast<f64x2*>(&Bs[buf ^ 1][sk * BG_LD + sc + v * 32]) = rb[v];
        }
      }
      lds_barrier();
    }
  }
  if (live) {
    double* Ob = p.Cout + ((size_t)bi * NBK - p.orow) * p.ldout + ((size_t)bj * NBK - p.ocol);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) Ob[(size_t)(mi * 16 + lk + 4 * r) * p.ldout + ni * 16 + lr] = acc[mi][ni][r];
  }
}

// Z_t[:, c] = sum_a X_t[:, a] * Dw[a, c] for the 64-row block t outside the pivot (blocks kb0 .. kb0 + m - 1) and the
// pivot's column block c; Dw = the full symmetric inverse of the pivot block ([64 m][64 m]).  Writes only the operand
// panels: XTW[c*64 + kk][t*64 + r] = s X[r][c*64 + kk], NZT[c*64 + col][t*64 + row] = -Z[row][col].
__global__ __launch_bounds__(256) void k_gj_panel_w(const double* __restrict__ A, int npad, int kb0, int m,
                                                    const double* __restrict__ Dw, double* __restrict__ NZT,
                                                    double* __restrict__ XTW, size_t ldx) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* As = sm;                  // X_t[:, a]  [64][LDA_S]
  double* Bs = sm + NBK * LDA_S;    // Dw[a, c]   [64][LDB_S]
  const int t = blockIdx.x, c = blockIdx.y;
  if (t >= kb0 && t < kb0 + m) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const bool upper = t < kb0;
  const double sgn = upper ? -1.0 : 1.0;
  const int ldd = m * NBK;
  f64x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[mi][ni][r] = 0.0;
  for (int a = 0; a < m; ++a) {
    for (int e = tid; e < NBK * NBK; e += 256) {
      const int r = e >> 6, cc = e & 63;
      if (upper)
        As[r * LDA_S + cc] = A[(size_t)(t * NBK + r) * npad + (size_t)(kb0 + a) * NBK + cc];       // X[r][cc]
      else
        As[cc * LDA_S + r] = A[(size_t)((kb0 + a) * NBK + r) * npad + (size_t)t * NBK + cc];       // X[cc][r]
    }
    load_tile(Bs, LDB_S, Dw + (size_t)a * NBK * ldd + (size_t)c * NBK, (size_t)ldd);
    lds_barrier();
    if (a == c)
      for (int e = tid; e < NBK * NBK; e += 256) {
        const int kk = e >> 6, r = e & 63;
        XTW[(size_t)(c * NBK + kk) * ldx + (size_t)t * NBK + r] = sgn * As[r * LDA_S + kk];
      }
    tile_mma64(As, Bs, acc);
    lds_barrier();
  }
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        As[(wr * 32 + mi * 16 + lk + 4 * r) * LDA_S + wc * 32 + ni * 16 + lr] = acc[mi][ni][r];     // Z[row][col]
  lds_barrier();
  for (int e = tid; e < NBK * NBK; e += 256) {
    const int kk = e >> 6, r = e & 63;
    NZT[(size_t)(c * NBK + kk) * ldx + (size_t)t * NBK + r] = -As[r * LDA_S + kk];
  }
}

// The pivot rows / columns after the step: block (t, kb0 + c) = -Z_t[:, c] for t above the pivot, block (kb0 + c, t) =
// Z_t[:, c]^T for t below it, and the pivot block itself = Dw (upper 64-blocks).
__global__ __launch_bounds__(256) void k_gj_wback_w(double* __restrict__ A, int npad, int kb0, int m,
                                                    const double* __restrict__ Dw, const double* __restrict__ NZT,
                                                    size_t ldx) {
  __shared__ double Ts[NBK * (NBK + 1)];
  const int t = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int ldd = m * NBK;
  if (t >= kb0 && t < kb0 + m) {
    const int a = t - kb0;
    if (a > c) return;
    for (int e = tid; e < NBK * NBK; e += 256) {
      const int r = e >> 6, cc = e & 63;
      A[(size_t)(t * NBK + r) * npad + (size_t)(kb0 + c) * NBK + cc] = Dw[(size_t)(a * NBK + r) * ldd + (size_t)c * NBK + cc];
    }
    return;
  }
  if (t < kb0) {
    for (int e = tid; e < NBK * NBK; e += 256) {
      const int kk = e >> 6, r = e & 63;
      Ts[kk * (NBK + 1) + r] = NZT[(size_t)(c * NBK + kk) * ldx + (size_t)t * NBK + r];      // -Z[r][kk]
    }
    __syncthreads();
    for (int e = tid; e < NBK * NBK; e += 256) {
      const int r = e >> 6, kk = e & 63;
      A[(size_t)(t * NBK + r) * npad + (size_t)(kb0 + c) * NBK + kk] = Ts[kk * (NBK + 1) + r];
    }
  } else {
    for (int e = tid; e < NBK * NBK; e += 256) {
      const int kk = e >> 6, r = e & 63;
      A[(size_t)((kb0 + c) * NBK + kk) * npad + (size_t)t * NBK + r] = -NZT[(size_t)(c * NBK + kk) * ldx + (size_t)t * NBK + r];
    }
  }
}

// the rank-64 sweep keeps the upper 64-block triangle: fill in the blocks below the diagonal (the finished inverse is
// symmetric)
__global__ __launch_bounds__(256) void k_mirror_blocks(double* __restrict__ D, int nd) {
  const size_t tot = (size_t)nd * nd;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / nd), j = (int)(e % nd);
    if ((i / NBK) > (j / NBK)) D[e] = D[(size_t)j * nd + i];
  }
}

}  // namespace effq

using namespace effq;

extern "C" {

// workspace of the rank-64 sweep on an npad x npad matrix that is already in place: XT [64][npad], NZ [npad][64], 2 Dinv
static size_t gj64_aux_doubles(size_t npad) { return 2 * (size_t)NBK * npad + 2 * NBK * NBK; }

// the wide sweep (pivot blocks of 256) from this many 64-blocks on.  Measured inside the calibration (ms per calibration,
// one box): rank-64 sweep everywhere 689.6; 256-row pivot blocks from n = 6400 on 671.0; 256-row (or 128-row, fused pivot
// launch) blocks for every n >= 512: 683.5 / 681.8 - below n ~ 5000 an inverse is a chain of dependent launches either
// way, and the rank-64 sweep has the shortest one.  Every wide sweep takes pivot blocks of WB = 4 64-blocks (the 128-row
// form with its fused pivot kernel measured slower and left the tree: DESIGN.md)
constexpr int GJ_WIDE_MIN_BLOCKS = 100;
static bool gj_takes_wide(int nblk) { return nblk >= GJ_WIDE_MIN_BLOCKS; }

size_t effq_spd_inverse_ws_bytes(int n) {
  if (n <= 0) return 0;
  const size_t npad = (size_t)round_up(n, NBK);
  size_t d = npad * npad + gj64_aux_doubles(npad);
  if (gj_takes_wide((int)(npad / NBK))) {
    const size_t ldx = (size_t)round_up((int)npad, BG_T);
    d = npad * npad + 2 * (size_t)WK * ldx + (size_t)WK * WK + gj64_aux_doubles(WK);
  }
  return d * sizeof(double) + 256;
}

int effq_ainv_ld(int n) { return n > 0 ? round_up(n, 32) : 0; }

// in-place rank-64 symmetric Gauss-Jordan sweep of the npad x npad matrix A64 (upper 64-block triangle kept)
static int gj64_sweep(double* A64, int npad, double* aux, hipStream_t st) {
  const int nblk = npad / NBK;
  double* XT = aux;                              // [64][npad]
  double* NZ = XT + (size_t)NBK * npad;          // [npad][64]
  double* Dinv = NZ + (size_t)NBK * npad;
  const size_t lds = (size_t)(NBK * LDA_S + NBK * LDB_S) * sizeof(double);
  // The trailing update of step k also forms the inverse of the NEXT pivot block (look-ahead workgroup, see
  // k_gj_trail_sym): only step 0 needs the stand-alone k_gj_diag.  Dinv is double-buffered by step parity.
  for (int k = 0; k < nblk; ++k) {
    const int kb = k * NBK;
    double* Dk = Dinv + (size_t)(k & 1) * NBK * NBK;
    double* Dn = Dinv + (size_t)((k + 1) & 1) * NBK * NBK;
    if (k == 0) hipLaunchKernelGGL(k_gj_diag, dim3(1), dim3(GJD_T), 0, st, A64, npad, kb, Dk);
    hipLaunchKernelGGL(k_gj_panel, dim3(nblk), dim3(256), lds, st, A64, npad, kb, Dk, NZ, XT);
    if (nblk > 1)
      hipLaunchKernelGGL(k_gj_trail_sym, dim3((nblk + GJ_CT - 1) / GJ_CT, nblk + 1), dim3(256), 0, st, A64, npad, kb, NZ,
                         XT, Dn);
    EFFQ_LAUNCH_CHECK();
  }
  return EFFQ_OK;
}

// helper stream + two events per (thread, caller stream): the next pivot block is inverted beside the big update
struct GjWideCtx {
  int dev;
  hipStream_t caller, helper;
  hipEvent_t e1, e2;
};
static thread_local std::vector<GjWideCtx> g_gj_ctx;

static int gj_wide_ctx(hipStream_t caller, GjWideCtx** out) {
  int dev = 0;
  EFFQ_HIP(hipGetDevice(&dev));
  for (GjWideCtx& c : g_gj_ctx)
    if (c.dev == dev && c.caller == caller) {
      *out = &c;
      return EFFQ_OK;
    }
  GjWideCtx c;
  c.dev = dev;
  c.caller = caller;
  int prio = 0;
  if (hipStreamGetPriority(caller, &prio) != hipSuccess) prio = 0;
  EFFQ_HIP(hipStreamCreateWithPriority(&c.helper, hipStreamNonBlocking, prio));
  EFFQ_HIP(hipEventCreateWithFlags(&c.e1, hipEventDisableTiming));
  EFFQ_HIP(hipEventCreateWithFlags(&c.e2, hipEventDisableTiming));
  g_gj_ctx.push_back(c);
  *out = &g_gj_ctx.back();
  return EFFQ_OK;
}

static int gj_wide_sweep(double* A64, int npad, double* aux, hipStream_t st) {
  const int nblk = npad / NBK;
  const size_t ldx = (size_t)round_up(npad, BG_T);
  double* NZT = aux;                               // [256][ldx]
  double* XTW = NZT + (size_t)WK * ldx;            // [256][ldx]
  double* Dw = XTW + (size_t)WK * ldx;             // [64 m][64 m]: the pivot block, then its inverse
  double* aux64 = Dw + (size_t)WK * WK;
  const int nK = (nblk + WB - 1) / WB, nm = (nblk + 1) / 2;
  GjWideCtx* ctx = nullptr;
  if (nK > 1) {
    const int rc = gj_wide_ctx(st, &ctx);
    if (rc != EFFQ_OK) return rc;
  }
  hipStream_t s2 = ctx ? ctx->helper : st;
  const size_t lds = (size_t)(NBK * LDA_S + NBK * LDB_S) * sizeof(double);
  auto pivot_block = [&](int k0, int mk, int kdim, hipStream_t s) -> int {
    // Dw = the pivot block (blocks k0 .. k0 + mk - 1) with the pending rank-kdim update applied, then inverted
    GjBig g;
    memset(&g, 0, sizeof(g));
    g.Cin = A64; g.ldin = (size_t)npad;
    g.Cout = Dw; g.ldout = (size_t)mk * NBK; g.orow = k0 * NBK; g.ocol = k0 * NBK;
    g.NZT = NZT; g.XTW = XTW; g.ldx = ldx; g.kdim = kdim; g.nblk = nblk;
    g.i0m = k0 / 2; g.j0m = k0 / 2;
    g.skip_lo = g.skip_hi = -1; g.la_lo = g.la_hi = -1;
    const int span = (mk + 1) / 2;
    hipLaunchKernelGGL(k_gj_big, dim3(span, span), dim3(256), 0, s, g);
    EFFQ_LAUNCH_CHECK();
    const int rc = gj64_sweep(Dw, mk * NBK, aux64, s);
    if (rc != EFFQ_OK) return rc;
    hipLaunchKernelGGL(k_mirror_blocks, dim3(64), dim3(256), 0, s, Dw, mk * NBK);
    EFFQ_LAUNCH_CHECK();
    return EFFQ_OK;
  };
  {
    const int rc = pivot_block(0, nblk < WB ? nblk : WB, 0, st);
    if (rc != EFFQ_OK) return rc;
  }
  for (int K = 0; K < nK; ++K) {
    const int kb0 = K * WB, m = (nblk - kb0 < WB) ? nblk - kb0 : WB;
    const int kn0 = kb0 + WB, mn = (K + 1 < nK) ? ((nblk - kn0 < WB) ? nblk - kn0 : WB) : 0;
    hipLaunchKernelGGL(k_gj_panel_w, dim3(nblk, m), dim3(256), lds, st, A64, npad, kb0, m, Dw, NZT, XTW, ldx);
    EFFQ_LAUNCH_CHECK();
    if (ctx) {
      EFFQ_HIP(hipEventRecord(ctx->e1, st));
      EFFQ_HIP(hipStreamWaitEvent(s2, ctx->e1, 0));
    }
    // (the write-back reads the inverse of THIS pivot block from Dw: before the next pivot block overwrites it.  It is
    // a copy of n x 64 m doubles; the pivot work behind it on the helper stream is the part that must not wait)
    hipLaunchKernelGGL(k_gj_wback_w, dim3(nblk, m), dim3(256), 0, s2, A64, npad, kb0, m, Dw, NZT, ldx);
    EFFQ_LAUNCH_CHECK();
    if (mn > 0) {
      const int rc = pivot_block(kn0, mn, m * NBK, s2);
      if (rc != EFFQ_OK) return rc;
    }
    if (nblk > m) {
      GjBig g;
      memset(&g, 0, sizeof(g));
      g.Cin = A64; g.ldin = (size_t)npad;
      g.Cout = A64; g.ldout = (size_t)npad; g.orow = 0; g.ocol = 0;
      g.NZT = NZT; g.XTW = XTW; g.ldx = ldx; g.kdim = m * NBK; g.nblk = nblk;
      g.i0m = 0; g.j0m = 0;
      g.skip_lo = kb0; g.skip_hi = kb0 + m;
      g.la_lo = mn > 0 ? kn0 : -1; g.la_hi = mn > 0 ? kn0 + mn : -1;
      hipLaunchKernelGGL(k_gj_big, dim3(nm, nm), dim3(256), 0, st, g);
      EFFQ_LAUNCH_CHECK();
    }
    if (ctx) {
      EFFQ_HIP(hipEventRecord(ctx->e2, s2));
      EFFQ_HIP(hipStreamWaitEvent(st, ctx->e2, 0));
    }
  }
  return EFFQ_OK;
}

// The helper stream of the 256-row sweep for `stream`, created NOW instead of at the first large inverse: streams take their
// hardware queue in the order they are created, and a communicator created in between (RCCL brings streams of its own)
// moved the calibration's streams onto shared queues (hip_ops.HipOps.warm_streams)
int effq_spd_inverse_prepare(void* stream) {
  GjWideCtx* ctx = nullptr;
  return gj_wide_ctx(as_stream(stream), &ctx);
}

int effq_spd_inverse(const float* A0, int n, int has_bias, double rho, double eta, float* Ainv, void* ws,
                     size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(A0 && Ainv && ws && n > 0);
  EFFQ_CHECK_ARG(eta > 0.0 && rho >= 0.0);
  if (ws_bytes < effq_spd_inverse_ws_bytes(n)) {
    set_error("spd_inverse: workspace %zu < required %zu", ws_bytes, effq_spd_inverse_ws_bytes(n));
    return EFFQ_ERR_WORKSPACE;
  }
  const int npad = round_up(n, NBK);
  double* A64 = reinterpret_cast<double*>(ws);
  double* aux = A64 + (size_t)npad * npad;
  hipStream_t st = as_stream(stream);
  {
    size_t nb = ((size_t)npad * npad + 255) / 256;
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(k_build_a64, dim3((unsigned)nb), dim3(256), 0, st, A0, n, npad, has_bias, rho, eta, A64);
    EFFQ_LAUNCH_CHECK();
  }
  const size_t lds = (size_t)(NBK * LDA_S + NBK * LDB_S) * sizeof(double);
  EFFQ_HIP(raise_lds_limit<k_gj_panel>(lds));
  EFFQ_HIP(raise_lds_limit<k_gj_panel_w>(lds));
  const int rc = gj_takes_wide(npad / NBK) ? gj_wide_sweep(A64, npad, aux, st) : gj64_sweep(A64, npad, aux, st);
  if (rc != EFFQ_OK) return rc;
  {
    const int lda = effq_ainv_ld(n);
    size_t nb = ((size_t)n * lda + 255) / 256;
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(k_a64_to_f32, dim3((unsigned)nb), dim3(256), 0, st, A64, n, npad, Ainv, lda);
    EFFQ_LAUNCH_CHECK();
  }
  return EFFQ_OK;
}

// which sweep effq_spd_inverse takes for n (launches nothing): *wide = the 256-row sweep, *nblk = 64-blocks per side,
// *pivot_blocks = elimination steps (nblk for the rank-64 sweep, the last one of a wide sweep may be shorter)
int effq_spd_inverse_plan(int n, int* wide, int* nblk, int* pivot_blocks) {
  EFFQ_CHECK_ARG(n > 0 && wide && nblk && pivot_blocks);
  const int nb = round_up(n, NBK) / NBK;
  *wide = gj_takes_wide(nb) ? 1 : 0;
  *nblk = nb;
  *pivot_blocks = *wide ? (nb + WB - 1) / WB : nb;
  return EFFQ_OK;
}

}  // extern "C"
