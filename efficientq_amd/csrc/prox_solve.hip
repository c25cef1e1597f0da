// Proximal step of the ADMM, second half: the right-hand side Bm and the per-iteration product  What = Bm * A^-1  on the
// matrix cores, with the fp32 inverse that spd_inverse.hip formed for the iteration's rho.
// Reference: solver.py:316-325 (getAB), :327-345 (solve; torch.linalg.solve = LU, every iteration).
#include "common.h"
#include "internal.h"
#include "project_dual.h"

namespace effq {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Bm[c2][ldb] = B0 + eta*[W0|b0] + rho*[G-dual|0]     (solver.py:316-322, fp32, reference op order: prox_rhs)
__global__ __launch_bounds__(256) void k_build_b(const float* __restrict__ B0, const float* __restrict__ W0,
                                                 const float* __restrict__ b0, const float* __restrict__ G,
                                                 const float* __restrict__ dual, int c2, int n, int has_bias,
                                                 float rho, float eta, float* __restrict__ Bm, int ldb, int c2p,
                                                 const float* __restrict__ wprev, float shift) {
  const size_t tot = (size_t)c2p * ldb;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const int nw = n - has_bias;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += stride) {
    const int r = (int)(e / ldb), k = (int)(e % ldb);
    float v = 0.0f;
    if (r < c2 && k < n) {
      if (k < nw) {
        const size_t wi = (size_t)r * nw + k;
        v = prox_rhs(B0[(size_t)r * n + k], W0[wi], G[wi], dual[wi], eta, rho);
        if (wprev != nullptr) v = v + shift * wprev[wi];     // effq_prox_solve_shifted: + d * W_prev * I'
      } else {
        v = B0[(size_t)r * n + k] + eta * b0[r];
      }
    }
    Bm[e] = v;
  }
}

// The same, four columns per thread (row per blockIdx.y): for weight rows that are a multiple of 4 long (every layer of the
// shipped nets but a 1-channel first conv) - 16-byte loads, no integer division per element.
__global__ __launch_bounds__(256) void k_build_b4(const float* __restrict__ B0, const float* __restrict__ W0,
                                                  const float* __restrict__ b0, const float* __restrict__ G,
                                                  const float* __restrict__ dual, int c2, int n, int has_bias,
                                                  float rho, float eta, float* __restrict__ Bm, int ldb,
                                                  const float* __restrict__ wprev, float shift) {
  __builtin_amdgcn_s_setprio(2);   // ADMM chain (critical path) over the loss / inverse streams

  const int r = blockIdx.y;
  const int nw = n - has_bias;
  float* out = Bm + (size_t)r * ldb;
  for (int k = (blockIdx.x * blockDim.x + threadIdx.x) * 4; k < ldb; k += gridDim.x * blockDim.x * 4) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < c2 && k < nw) {                       // nw % 4 == 0: a group of four never straddles the bias column
      const size_t wi = (size_t)r * nw + k;
      const float* bp = B0 + (size_t)r * n + k;   // (rows of B0 are n long: not 16-byte aligned in general)
      const float4 w0 = *reinterpret_cast<const float4*>(W0 + wi), g = *reinterpret_cast<const float4*>(G + wi),
                   du = *reinterpret_cast<const float4*>(dual + wi);
      v.x = prox_rhs(bp[0], w0.x, g.x, du.x, eta, rho);
      v.y = prox_rhs(bp[1], w0.y, g.y, du.y, eta, rho);
      v.z = prox_rhs(bp[2], w0.z, g.z, du.z, eta, rho);
      v.w = prox_rhs(bp[3], w0.w, g.w, du.w, eta, rho);
      if (wprev != nullptr) {
        const float4 wp = *reinterpret_cast<const float4*>(wprev + wi);
        v.x = v.x + shift * wp.x;
        v.y = v.y + shift * wp.y;
        v.z = v.z + shift * wp.z;
        v.w = v.w + shift * wp.w;
      }
    } else if (r < c2 && k == nw && has_bias) {
      v.x = B0[(size_t)r * n + k] + eta * b0[r];
    }
    *reinterpret_cast<float4*>(out + k) = v;
  }
}

__global__ __launch_bounds__(256) void k_prox_reduce4(const float* __restrict__ part, int ldp, int nsplit, int c2, int n,
                                                      int has_bias, float* __restrict__ wstar, float* __restrict__ bstar) {
  __builtin_amdgcn_s_setprio(2);   // ADMM chain (critical path) over the loss / inverse streams

  const int r = blockIdx.y;
  const int nw = n - has_bias;
  const size_t tot = (size_t)c2 * ldp;
  const float* row = part + (size_t)r * ldp;
  for (int k = (blockIdx.x * blockDim.x + threadIdx.x) * 4; k < ldp; k += gridDim.x * blockDim.x * 4) {
    if (k >= n) continue;
    float4 v = *reinterpret_cast<const float4*>(row + k);
    for (int z = 1; z < nsplit; ++z) {            // slice order: deterministic
      const float4 t = *reinterpret_cast<const float4*>(row + (size_t)z * tot + k);
      v.x += t.x;
      v.y += t.y;
      v.z += t.z;
      v.w += t.w;
    }
    if (k < nw)
      *reinterpret_cast<float4*>(wstar + (size_t)r * nw + k) = v;
    else
      bstar[r] = v.x;
  }
}

// What = Bm * Ainv on the f32 matrix cores.  Ainv is exactly symmetric, so What[r][c] = sum_k Bm[r][k] *
// Ainv[c][k]: BOTH operands are read along K (contiguous, 16-byte loads), staged as [row][32+4] tiles in
// LDS (conflict-free ds_read_b128, 4 MFMAs per pair of reads) with the next K tile prefetched into
// registers under the MFMAs of the current one.  Wave tile = (32*MT) x (32*NTN); workgroup tile =
// (32*MT*WM) x (32*NTN*WN), 4 waves.
constexpr int PBK = 32, PLD = PBK + 4;

template <int MT, int WM, int WN, int NTN>
__global__ __launch_bounds__(256) void k_prox_gemm(const float* __restrict__ Bm, int ldb, const float* __restrict__ Ainv,
                                                   int lda, int n, int c2, int has_bias, float* __restrict__ wstar,
                                                   float* __restrict__ bstar, float* __restrict__ part, int ldp) {
  __builtin_amdgcn_s_setprio(2);   // ADMM chain (critical path) over the loss / inverse streams

  constexpr int BM = 32 * MT * WM, BN = 32 * WN * NTN;
  constexpr int NA = BM * 8 / 256, NB = BN * 8 / 256;   // 16-byte loads per thread per K tile
  static_assert(WM * WN == 4 && NA >= 1 && NB >= 1, "4 waves");
  __shared__ __attribute__((aligned(16))) float As[BM * PLD];
  __shared__ __attribute__((aligned(16))) float Bs[BN * PLD];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wid / WN, wn = wid % WN;
  const int row0 = blockIdx.y * BM, col0 = blockIdx.x * BN;

  f32x16 acc[MT][NTN];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < NTN; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.0f;

  // The prefetch is written out twice (prologue and loop) rather than as a lambda over ra/rb: captured by
  // reference the arrays stay in scratch memory and every prefetch is waited for and spilled on the spot.
  // Columns >= n are clamped (their outputs are dropped below): an unconditional load keeps the prefetch
  // asynchronous, a branch around it makes hipcc wait for it inside the branch.
  f32x4 ra[NA], rb[NB];
  const float* pa[NA];
  const float* pb[NB];
#pragma unroll
  for (int q = 0; q < NA; ++q) {
    const int u = tid + q * 256, r = u >> 3, c4 = u & 7;
    pa[q] = Bm + (size_t)(row0 + r) * ldb + c4 * 4;   // Bm is zero padded
  }
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int u = tid + q * 256, r = u >> 3, c4 = u & 7;
    pb[q] = Ainv + (size_t)min(col0 + r, n - 1) * lda + c4 * 4;   // lda padded
  }
#define EFFQ_PROX_FETCH(k0)                                                         \
  {                                                                                 \
    _Pragma("unroll") for (int q = 0; q < NA; ++q)                                  \
        ra[q] = *reinterpret_cast<const f32x4*>(pa[q] + (k0));                      \
    _Pragma("unroll") for (int q = 0; q < NB; ++q)                                  \
        rb[q] = *reinterpret_cast<const f32x4*>(pb[q] + (k0));                      \
  }
  // split K: slice z of gridDim.z takes K tiles [kt0, kt1); with more than one slice the partial tile goes
  // to part[z] and k_prox_reduce adds the slices in a fixed order
  const int nkt = ldb / PBK;   // ldb is a multiple of 32
  const int kt0 = (int)(((long long)nkt * blockIdx.z) / gridDim.z);
  const int nk = (int)(((long long)nkt * (blockIdx.z + 1)) / gridDim.z);
  EFFQ_PROX_FETCH(kt0 * PBK)
  for (int kt = kt0; kt < nk; ++kt) {
    lds_barrier();
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      const int u = tid + q * 256;
      *reinterpret_cast<f32x4*>(&As[(u >> 3) * PLD + (u & 7) * 4]) = ra[q];
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const int u = tid + q * 256;
      *reinterpret_cast<f32x4*>(&Bs[(u >> 3) * PLD + (u & 7) * 4]) = rb[q];
    }
    lds_barrier();
    EFFQ_PROX_FETCH(min(kt + 1, nk - 1) * PBK)   // unconditional: the last one is a harmless re-read
    __builtin_amdgcn_sched_barrier(0);           // keep the loads ahead of the MFMAs they hide under
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 a[MT], b[NTN];
#pragma unroll
      for (int m = 0; m < MT; ++m)
        a[m] = *reinterpret_cast<const f32x4*>(&As[((wm * MT + m) * 32 + li) * PLD + q * 8 + 4 * lh]);
#pragma unroll
      for (int t = 0; t < NTN; ++t)
        b[t] = *reinterpret_cast<const f32x4*>(&Bs[((wn * NTN + t) * 32 + li) * PLD + q * 8 + 4 * lh]);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NTN; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][e], b[t][e], acc[m][t], 0, 0, 0);
    }
  }
#undef EFFQ_PROX_FETCH
  const int nw = n - has_bias;
  if (gridDim.z > 1) {
    float* P = part + (size_t)blockIdx.z * c2 * ldp;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int t = 0; t < NTN; ++t) {
        const int col = col0 + (wn * NTN + t) * 32 + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = row0 + (wm * MT + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (row < c2 && col < n) P[(size_t)row * ldp + col] = acc[m][t][r];
        }
      }
    return;
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < NTN; ++t) {
      const int col = col0 + (wn * NTN + t) * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + (wm * MT + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row < c2 && col < n) {
          if (col < nw)
            wstar[(size_t)row * nw + col] = acc[m][t][r];
          else
            bstar[row] = acc[m][t][r];
        }
      }
    }
}


// ---- the same product on the bf16 matrix cores with both operands split in three --------------------------------
// An fp32 value x is the exact sum of three bf16 values x1 + x2 + x3 (8 + 8 + 8 mantissa bits; bf16 has fp32's
// exponent range, so no scaling is needed).  x y = sum_{i,j} x_i y_j; the six products with i + j <= 4 carry everything
// down to 2^-24 of x y - the size of the rounding of an fp32 product itself - and each is EXACT in the fp32 accumulator
// of v_mfma_f32_32x32x16_bf16 (8 x 8 bits).  Six bf16 MFMAs (32 x 32 x 16 each, 32 cycles) replace eight fp32 MFMAs
// (32 x 32 x 2, 64 cycles) per K = 16: 0.375 of the matrix-core time for the same fp32-grade result.  The operands are
// split ON THE FLY while a K tile is staged into LDS (3 planes of [rows][32 + 8] bf16, conflict-free b128 fragment
// reads), so HBM / L2 still carry 4 bytes per element and nothing upstream changes.
// Workgroup tile (128 MT_) x 256, 8 waves as WM_ x WN_; K tiles of 32; split K like k_prox_gemm.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
constexpr int B3_K = 16;                       // K tile = one MFMA step
constexpr int B3_LD = B3_K + 8;                // bf16 elements per LDS row (48 bytes: conflict-free b128 fragment reads)

__device__ __forceinline__ void split3(const f32x4 v, bf16x4& p0, bf16x4& p1, bf16x4& p2) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const __bf16 b0 = (__bf16)v[e];
    const float r1 = v[e] - (float)b0;          // exact
    const __bf16 b1 = (__bf16)r1;
    const float r2 = r1 - (float)b1;            // exact
    p0[e] = b0;
    p1[e] = b1;
    p2[e] = (__bf16)r2;
  }
}

// Two LDS stages: while the MFMAs of K tile kt read stage kt & 1, the tile kt + 1 (fetched into registers one
// iteration earlier) is split and stored into the other stage and the global loads of tile kt + 2 are issued - one
// barrier per K tile, the conversion and the loads hide under the matrix-core work of the co-resident waves.
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(512) void k_prox_gemm_b3(const float* __restrict__ Bm, int ldb, const float* __restrict__ Ainv,
                                                      int lda, int n, int c2, int has_bias, float* __restrict__ wstar,
                                                      float* __restrict__ bstar, float* __restrict__ part, int ldp) {
  __builtin_amdgcn_s_setprio(2);   // ADMM chain (critical path) over the loss / inverse streams
  constexpr int MT = BM / WM / 32, NT = BN / WN / 32;
  constexpr int NA = BM * 4 / 512, NB = BN * 4 / 512;          // 16-byte global loads per thread per K tile
  constexpr int STAGE = 3 * (BM + BN) * B3_LD;                  // bf16 elements per stage
  static_assert(WM * WN == 8 && MT >= 1 && NT >= 1 && NA >= 1 && NB >= 1, "8 waves");
  extern __shared__ __attribute__((aligned(16))) unsigned char b3_lds[];
  __bf16* lds = reinterpret_cast<__bf16*>(b3_lds);              // [2][ As [3][BM][B3_LD] | Bs [3][BN][B3_LD] ]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wid / WN, wn = wid % WN;
  const int row0 = blockIdx.y * BM, col0 = blockIdx.x * BN;

  f32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.0f;

  f32x4 ra[NA], rb[NB];
  const float* pa[NA];
  const float* pb[NB];
#pragma unroll
  for (int q = 0; q < NA; ++q) {
    const int u = tid + q * 512, r = u >> 2, c4 = u & 3;
    pa[q] = Bm + (size_t)(row0 + r) * ldb + c4 * 4;             // Bm is zero padded to the row tile
  }
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int u = tid + q * 512, r = u >> 2, c4 = u & 3;
    pb[q] = Ainv + (size_t)min(col0 + r, n - 1) * lda + c4 * 4; // lda padded; columns >= n are dropped below
  }
#define EFFQ_B3_FETCH(k0)                                                           \
  {                                                                                 \
    _Pragma("unroll") for (int q = 0; q < NA; ++q)                                  \
        ra[q] = *reinterpret_cast<const f32x4*>(pa[q] + (k0));                      \
    _Pragma("unroll") for (int q = 0; q < NB; ++q)                                  \
        rb[q] = *reinterpret_cast<const f32x4*>(pb[q] + (k0));                      \
  }
#define EFFQ_B3_STORE(stage)                                                                        \
  {                                                                                                 \
    __bf16* As_ = lds + (stage) * STAGE;                                                            \
    __bf16* Bs_ = As_ + 3 * BM * B3_LD;                                                             \
    _Pragma("unroll") for (int q = 0; q < NA; ++q) {                                                \
      const int u = tid + q * 512, off = (u >> 2) * B3_LD + (u & 3) * 4;                            \
      bf16x4 p0, p1, p2;                                                                            \
      split3(ra[q], p0, p1, p2);                                                                    \
      *reinterpret_cast<bf16x4*>(&As_[off]) = p0;                                                   \
      *reinterpret_cast<bf16x4*>(&As_[BM * B3_LD + off]) = p1;                                      \
      *reinterpret_cast<bf16x4*>(&As_[2 * BM * B3_LD + off]) = p2;                                  \
    }                                                                                               \
    _Pragma("unroll") for (int q = 0; q < NB; ++q) {                                                \
      const int u = tid + q * 512, off = (u >> 2) * B3_LD + (u & 3) * 4;                            \
      bf16x4 p0, p1, p2;                                                                            \
      split3(rb[q], p0, p1, p2);                                                                    \
      *reinterpret_cast<bf16x4*>(&Bs_[off]) = p0;                                                   \
      *reinterpret_cast<bf16x4*>(&Bs_[BN * B3_LD + off]) = p1;                                      \
      *reinterpret_cast<bf16x4*>(&Bs_[2 * BN * B3_LD + off]) = p2;                                  \
    }                                                                                               \
  }
  const int nkt = ldb / B3_K;                   // ldb is a multiple of 32
  const int kt0 = (int)(((long long)nkt * blockIdx.z) / gridDim.z);
  const int nk = (int)(((long long)nkt * (blockIdx.z + 1)) / gridDim.z);
  EFFQ_B3_FETCH(kt0 * B3_K)
  EFFQ_B3_STORE(0)
  EFFQ_B3_FETCH(min(kt0 + 1, nk - 1) * B3_K)
  lds_barrier();
  for (int kt = kt0; kt < nk; ++kt) {
    const int st = (kt - kt0) & 1;
    if (kt + 1 < nk) EFFQ_B3_STORE(st ^ 1)       // tile kt + 1 (in registers since the previous iteration)
    EFFQ_B3_FETCH(min(kt + 2, nk - 1) * B3_K)    // unconditional: past the end a harmless re-read
    const __bf16* As = lds + st * STAGE;
    const __bf16* Bs = As + 3 * BM * B3_LD;
    bf16x8 a[MT][3], b[NT][3];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        a[m][p] = *reinterpret_cast<const bf16x8*>(&As[p * BM * B3_LD + ((wm * MT + m) * 32 + li) * B3_LD + 8 * lh]);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        b[t][p] = *reinterpret_cast<const bf16x8*>(&Bs[p * BN * B3_LD + ((wn * NT + t) * 32 + li) * B3_LD + 8 * lh]);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        // smallest terms first (x1 y3, x2 y2, x3 y1), then x1 y2, x2 y1, then x1 y1
        acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m][0], b[t][2], acc[m][t], 0, 0, 0);
        acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m][1], b[t][1], acc[m][t], 0, 0, 0);
        acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m][2], b[t][0], acc[m][t], 0, 0, 0);
        acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m][0], b[t][1], acc[m][t], 0, 0, 0);
        acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m][1], b[t][0], acc[m][t], 0, 0, 0);
        acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m][0], b[t][0], acc[m][t], 0, 0, 0);
      }
    lds_barrier();                               // stage st has been read by every wave, stage st ^ 1 is complete
  }
#undef EFFQ_B3_FETCH
#undef EFFQ_B3_STORE
  const int nw = n - has_bias;
  float* P = (gridDim.z > 1) ? part + (size_t)blockIdx.z * c2 * ldp : nullptr;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = col0 + (wn * NT + t) * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + (wm * MT + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row < c2 && col < n) {
          if (P != nullptr)
            P[(size_t)row * ldp + col] = acc[m][t][r];
          else if (col < nw)
            wstar[(size_t)row * nw + col] = acc[m][t][r];
          else
            bstar[row] = acc[m][t][r];
        }
      }
    }
}

// What = sum_z part[z] in slice order (deterministic), scattered to [wstar | bstar]
__global__ __launch_bounds__(256) void k_prox_reduce(const float* __restrict__ part, int ldp, int nsplit, int c2, int n,
                                                     int has_bias, float* __restrict__ wstar, float* __restrict__ bstar) {
  const size_t tot = (size_t)c2 * ldp, stride = (size_t)gridDim.x * blockDim.x;
  const int nw = n - has_bias;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += stride) {
    const int row = (int)(e / ldp), col = (int)(e % ldp);
    if (col >= n) continue;
    float v = part[e];
    for (int z = 1; z < nsplit; ++z) v += part[(size_t)z * tot + e];
    if (col < nw)
      wstar[(size_t)row * nw + col] = v;
    else
      bstar[row] = v;
  }
}

// workgroup tile variant and K split of the prox GEMM: ~440 workgroups, >= 6 K tiles per slice (measured
// best on MI355X for the BraTS sizes: scripts/prof_prox.py, forcing the split).  The 256-row variant holds 3
// workgroups per CU (104 VGPR + 64 AGPR, 45 KB LDS): ~760 workgroups fill the 768 slots evenly - with 545 some CUs
// carried 3 and others 2 (c2 = 256, n = 6913: 325 -> 266 us per solve).
//
// The variants (the values effq_prox_plan_query reports), each stated once with the template parameters of its kernel:
// the plan takes the grid from bm / bn, the launcher the kernel, its workgroup size and its dynamic LDS.
enum ProxVariant { PROX_F32_256 = 0, PROX_F32_128 = 1, PROX_F32_64 = 2, PROX_F32_32 = 3, PROX_B3_256 = 5, PROX_B3_128 = 7 };
typedef void (*ProxGemm)(const float*, int, const float*, int, int, int, int, float*, float*, float*, int);
struct ProxTile {
  ProxVariant variant;
  int bm, bn, threads;                 // workgroup tile (rows of Bm x columns of What), workgroup size
  size_t lds;                          // dynamic LDS: the two stages of k_prox_gemm_b3; 0 for k_prox_gemm (static)
  ProxGemm kernel;
  hipError_t (*raise_lds)(size_t);     // NULL where lds == 0
};
template <int MT, int WM, int WN, int NTN>
static ProxTile f32_tile(ProxVariant v) {
  return ProxTile{v, 32 * MT * WM, 32 * WN * NTN, 256, 0, k_prox_gemm<MT, WM, WN, NTN>, nullptr};
}
template <int BM, int BN, int WM, int WN>
static ProxTile b3_tile(ProxVariant v) {
  return ProxTile{v, BM, BN, 512, (size_t)2 * 3 * (BM + BN) * B3_LD * sizeof(__bf16), k_prox_gemm_b3<BM, BN, WM, WN>,
                  raise_lds_limit<k_prox_gemm_b3<BM, BN, WM, WN>>};
}
static const ProxTile TILE_F32_256 = f32_tile<2, 4, 1, 2>(PROX_F32_256);     // 256 x 64, waves 64 x 64
static const ProxTile TILE_F32_128 = f32_tile<1, 4, 1, 2>(PROX_F32_128);     // 128 x 64, waves 32 x 64
static const ProxTile TILE_F32_64 = f32_tile<1, 2, 2, 1>(PROX_F32_64);       // 64 x 64, waves 32 x 32
static const ProxTile TILE_F32_32 = f32_tile<1, 1, 4, 1>(PROX_F32_32);       // 32 x 128, waves 32 x 32
static const ProxTile TILE_B3_256 = b3_tile<256, 256, 4, 2>(PROX_B3_256);
static const ProxTile TILE_B3_128 = b3_tile<128, 128, 2, 4>(PROX_B3_128);

struct ProxPlan {
  const ProxTile* tile;
  int gx, gy, nsplit, c2p, ldb;
};
static ProxPlan prox_plan(int c2, int n) {
  ProxPlan p;
  p.c2p = (c2 > 128) ? round_up(c2, 256) : (c2 > 64) ? 128 : round_up(c2, 32);
  p.ldb = round_up(n, 32);
  const bool b3 = p.c2p >= 128 && n >= 1024;
  // bf16 matrix cores: 256 x 256 tiles, one workgroup of 8 waves per CU; 128 rows: 128 x 128 tiles (28 column tiles x 9 K
  // slices at n = 3457: half the partial slabs of the 128 x 256 tiling, two workgroups per CU): 37.7 against 43.1 us
  // alone, 35.8 against 44.3 in situ
  if (b3) p.tile = (p.c2p == 128) ? &TILE_B3_128 : &TILE_B3_256;
  else p.tile = (p.c2p >= 256) ? &TILE_F32_256 : (p.c2p == 128) ? &TILE_F32_128 : (p.c2p == 64) ? &TILE_F32_64 : &TILE_F32_32;
  p.gx = (n + p.tile->bn - 1) / p.tile->bn;
  p.gy = p.c2p / p.tile->bm;
  const int tiles = p.gx * p.gy;
  if (b3) {
    // K split so that the grid is about one round of the 256 CUs, at least 16 K tiles per slice
    const int nkt5 = p.ldb / B3_K;
    int s5 = (256 + tiles / 2) / tiles;
    if (s5 > nkt5 / 16) s5 = nkt5 / 16;
    if (s5 < 1) s5 = 1;
    p.nsplit = s5;
    return p;
  }
  const int nkt = p.ldb / PBK;
  int s = (440 + tiles - 1) / tiles;
  if (s > nkt / 6) s = nkt / 6;
  if (s > 16) s = 16;
  if (s < 1) s = 1;
  if (p.tile == &TILE_F32_256) {
    // fill the 768 slots (3 workgroups per CU) in whole rounds: the split with the best fill, smaller splits preferred
    const int smax = s > 1 ? 16 : 1;
    double best = -1.0;
    for (int c = 1; c <= smax && c <= nkt / 6; ++c) {
      const int wgs = tiles * c, rounds = (wgs + 767) / 768;
      const double score = (double)wgs / (768.0 * rounds) - 0.01 * c;
      if (score > best) { best = score; s = c; }
    }
  }
  p.nsplit = s;
  return p;
}

}  // namespace effq

using namespace effq;

extern "C" {

// the kernel variant, grid and K split effq_prox_solve* takes for (c2, n) (launches nothing)
int effq_prox_plan_query(int c2, int n, int* variant, int* gx, int* gy, int* nsplit) {
  EFFQ_CHECK_ARG(c2 > 0 && n > 0 && variant && gx && gy && nsplit);
  const ProxPlan p = prox_plan(c2, n);
  *variant = p.tile->variant;
  *gx = p.gx;
  *gy = p.gy;
  *nsplit = p.nsplit;
  return EFFQ_OK;
}

size_t effq_prox_ws_bytes(int c2, int n) {
  if (c2 <= 0 || n <= 0) return 0;
  const ProxPlan p = prox_plan(c2, n);
  return ((size_t)p.c2p + (p.nsplit > 1 ? (size_t)p.nsplit * c2 : 0)) * p.ldb * sizeof(float) + 256;
}

// Bm of one term: rows padded to the workgroup tile, K to the 32-wide K tile (zero filled).  wprev: the previous term of
// the shifted solve, or NULL
static int launch_build(const ProxSolve& s, const ProxPlan& pl, float* Bm, const float* wprev, hipStream_t st) {
  const int hb = s.has_bias ? 1 : 0;
  if (((s.n - hb) % 4) == 0) {
    const unsigned bx = (unsigned)((pl.ldb / 4 + 255) / 256);
    hipLaunchKernelGGL(k_build_b4, dim3(bx, (unsigned)pl.c2p), dim3(256), 0, st, s.B0, s.W0, s.b0, s.G, s.dual, s.c2, s.n,
                       hb, (float)s.rho, (float)s.eta, Bm, pl.ldb, wprev, (float)s.shift);
  } else {
    size_t nb = ((size_t)pl.c2p * pl.ldb + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_build_b, dim3((unsigned)nb), dim3(256), 0, st, s.B0, s.W0, s.b0, s.G, s.dual, s.c2, s.n, hb,
                       (float)s.rho, (float)s.eta, Bm, pl.ldb, pl.c2p, wprev, (float)s.shift);
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// the product: into wstar / bstar, or with more than one K slice into part
static int launch_gemm(const ProxSolve& s, const ProxPlan& pl, const float* Bm, float* part, hipStream_t st) {
  const ProxTile& t = *pl.tile;
  if (t.lds > 0) EFFQ_HIP(t.raise_lds(t.lds));
  hipLaunchKernelGGL(t.kernel, dim3(pl.gx, pl.gy, pl.nsplit), dim3(t.threads), t.lds, st, Bm, pl.ldb, s.Ainv,
                     effq_ainv_ld(s.n), s.n, s.c2, s.has_bias ? 1 : 0, s.wstar, s.bstar, part, pl.ldb);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// wstar / bstar = the K slices of part added up in slice order
static int launch_reduce(const ProxSolve& s, const ProxPlan& pl, const float* part, hipStream_t st) {
  const int hb = s.has_bias ? 1 : 0;
  if (((s.n - hb) % 4) == 0) {
    const unsigned bx = (unsigned)((pl.ldb / 4 + 255) / 256);
    hipLaunchKernelGGL(k_prox_reduce4, dim3(bx, (unsigned)s.c2), dim3(256), 0, st, part, pl.ldb, pl.nsplit, s.c2, s.n, hb,
                       s.wstar, s.bstar);
  } else {
    size_t nb = ((size_t)s.c2 * pl.ldb + 255) / 256;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(k_prox_reduce, dim3((unsigned)nb), dim3(256), 0, st, part, pl.ldb, pl.nsplit, s.c2, s.n, hb,
                       s.wstar, s.bstar);
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// internal (admm_run.hip; internal.h): the one place that checks the arguments and enqueues a prox solve
int effq_prox_enqueue(const ProxSolve* sp, void* stream) {
  EFFQ_CHECK_ARG(sp != nullptr);
  const ProxSolve& s = *sp;
  EFFQ_CHECK_ARG(s.B0 && s.Ainv && s.W0 && s.G && s.dual && s.wstar && s.ws && s.c2 > 0 && s.n > 0 && s.nterms >= 1);
  EFFQ_CHECK_ARG(!s.has_bias || (s.b0 != nullptr && s.bstar != nullptr));
  if (s.ws_bytes < effq_prox_ws_bytes(s.c2, s.n)) {
    set_error("prox_solve: workspace %zu < required %zu", s.ws_bytes, effq_prox_ws_bytes(s.c2, s.n));
    return EFFQ_ERR_WORKSPACE;
  }
  const ProxPlan pl = prox_plan(s.c2, s.n);
  float* Bm = reinterpret_cast<float*>(s.ws);
  float* part = Bm + (size_t)pl.c2p * pl.ldb;
  hipStream_t st = as_stream(stream);
  for (int term = 0; term < s.nterms; ++term) {
    if (!(s.prebuilt && term == 0))     // prebuilt: the previous projection already left Bm (ProjNext)
      if (const int rc = launch_build(s, pl, Bm, (term > 0) ? s.wstar : nullptr, st); rc != EFFQ_OK) return rc;
    if (const int rc = launch_gemm(s, pl, Bm, part, st); rc != EFFQ_OK) return rc;
    if (s.parts != nullptr)             // the caller's next kernel adds the K slices up itself
      *s.parts = ProxParts{(pl.nsplit > 1) ? part : nullptr, pl.nsplit, pl.ldb};
    else if (pl.nsplit > 1)
      if (const int rc = launch_reduce(s, pl, part, st); rc != EFFQ_OK) return rc;
  }
  return EFFQ_OK;
}

int effq_prox_solve(const float* B0, const float* Ainv, const float* W0, const float* b0, const float* G,
                    const float* dual, int c2, int n, int has_bias, double rho, double eta, float* wstar, float* bstar,
                    void* ws, size_t ws_bytes, void* stream) {
  const ProxSolve s = {B0, Ainv, W0, b0, G, dual, c2, n, has_bias, rho, eta, 0.0, 1, false, wstar, bstar, ws, ws_bytes,
                       nullptr};
  return effq_prox_enqueue(&s, stream);
}

int effq_prox_solve_shifted(const float* B0, const float* Ainv, const float* W0, const float* b0, const float* G,
                            const float* dual, int c2, int n, int has_bias, double rho, double eta, double rho_inv,
                            int nterms, float* wstar, float* bstar, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(rho_inv >= rho && rho > 0.0 && eta >= 0.0);
  const ProxSolve s = {B0, Ainv, W0, b0, G, dual, c2, n, has_bias, rho, eta, rho_inv - rho, nterms, false, wstar, bstar,
                       ws, ws_bytes, nullptr};
  return effq_prox_enqueue(&s, stream);
}

// internal (admm_run.hip): Bm = the start of the prox workspace, its row length
float* effq_prox_bm(void* ws, int c2, int n, int* ldb) {
  *ldb = prox_plan(c2, n).ldb;
  return reinterpret_cast<float*>(ws);
}

}  // extern "C"

