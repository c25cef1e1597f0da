// What the two distance transforms share (seg_surface.hip in integers, seg_surface_mm.hip with per-axis weights): the
// surface stencil on the decision bits of seg_masks.h, where the sites of a plane come from, and the three separable
// passes themselves, written once over a metric M (EdtVox, EdtMm):
//
//   rows     along w, one wave per row: the cost of the offset to the nearest site of the row, from the ballots of the
//            row's chunks of 64 (a sweep from the right records the next site after every chunk, a sweep from the left
//            writes each voxel once)
//   lines    along h, then along d: the lower envelope min_j (g(j) + cost(|i - j|)) of every line.  A slab of `tw` lines
//            adjacent along w is staged in LDS (every global access is a run of tw consecutive words), the first and last
//            finite entry of each line are noted, and every voxel searches outwards from itself inside that range until
//            the cost of the offset reaches its best value so far.  In place: a workgroup owns its lines.
#pragma once
#include <cmath>

#include "common.h"
#include "seg_masks.h"

namespace effq {

// slab of the line passes: tw lines adjacent along w are narrowed down until (n + 2) * tw words fit this.  32 KB keeps
// five workgroups on a compute unit (DESIGN section 13 measured the integer passes with it); a line longer than 2046
// leaves one line per workgroup
constexpr int EDT_LDS_AIM = 32 * 1024;

// the surface bits of one case: a voxel of a mask is a surface voxel when a face neighbour is background or lies outside
// the volume; all 2 C masks at once on the decision bits.  Shared by the integer and the weighted distance transform
// (seg_surface.hip, seg_surface_mm.hip): one definition of S(M).  Internal linkage: each of the two files has its own.
static __global__ __launch_bounds__(CC_THREADS) void k_surf_bits(const uint16_t* __restrict__ bits,
                                                          uint16_t* __restrict__ surf, int D, int H, int W) {
  const int S = D * H * W, HW = H * W;
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)i;
    const uint32_t b = bits[v];
    uint32_t inner = 0;
    if (b) {
      const int w = v % W, q = v / W, h = q % H, d = q / H;
      inner = b;
      inner &= w > 0 ? bits[v - 1] : 0u;
      inner &= w < W - 1 ? bits[v + 1] : 0u;
      inner &= h > 0 ? bits[v - W] : 0u;
      inner &= h < H - 1 ? bits[v + W] : 0u;
      inner &= d > 0 ? bits[v - HW] : 0u;
      inner &= d < D - 1 ? bits[v + HW] : 0u;
    }
    surf[v] = (uint16_t)(b & ~inner);
  }
}

// where the sites of plane q come from: P masks of uint8, or bit cc_plane_bit(q, C) of the surface bits
struct EdtSrc {
  const uint8_t* masks;
  const uint16_t* surf;
  int C;
};

__device__ __forceinline__ bool edt_site(const EdtSrc& s, int plane, int S, int idx) {
  if (s.surf) return (s.surf[idx] >> cc_plane_bit(plane, s.C)) & 1;
  return s.masks[(size_t)plane * S + idx] != 0;
}

// ---- the metrics ----------------------------------------------------------------------------------------------------
// A metric gives the stored word T, the type the candidates are formed in, the weight of an axis, the value of "no site",
// the cost of an offset of d voxels along an axis, and how a candidate g + c is formed and compared.  The expressions are
// the definition of the result (include/effq_hip.h): the weighted ones are fp32 term by term, none is reordered.
constexpr int EDT_INF = INT32_MAX;

struct EdtUnit {};                                     // the weight of an axis in voxel units: none

// squared distance in voxels, exact in integers.  A candidate is formed in uint32: EDT_INF + d^2 < 2^32
struct EdtVox {
  using T = int;
  using Acc = uint32_t;
  using Weight = EdtUnit;
  static constexpr int MAX_CHUNKS = 728;               // chunks of 64 of the longest row (W^2 < 2^31: W <= 46340)
  static __device__ __forceinline__ T none() { return EDT_INF; }
  static __device__ __forceinline__ bool finite(T g) { return g != EDT_INF; }
  static __device__ __forceinline__ Acc cost(Weight, int d) { return (Acc)(d * d); }
  static __device__ __forceinline__ Acc relax(Acc best, T g, Acc c) { return min(best, (Acc)g + c); }
};

// squared distance with per-axis weights: fl(g + fl(wa d^2)), d^2 < 2^24 exact as a float
struct EdtMm {
  using T = float;
  using Acc = float;
  using Weight = float;
  static constexpr int MAX_CHUNKS = EFFQ_EDT_MM_MAX_EXTENT / 64;
  static __device__ __forceinline__ T none() { return INFINITY; }
  static __device__ __forceinline__ bool finite(T g) { return g < INFINITY; }
  static __device__ __forceinline__ Acc cost(Weight wa, int d) { return wa * (float)(d * d); }
  static __device__ __forceinline__ Acc relax(Acc best, T g, Acc c) {
    const float cand = g + c;
    return cand < best ? cand : best;
  }
};

constexpr int EDT_THREADS = 256;
constexpr int EDT_ROWS = EDT_THREADS / 64;             // rows of one workgroup of the w pass: one per wave

// ---- rows -----------------------------------------------------------------------------------------------------------
template <class M>
__global__ __launch_bounds__(EDT_THREADS) void k_edt_rows(EdtSrc src, typename M::T* __restrict__ sq, int S, int W,
                                                          int nrows, typename M::Weight ww) {
  __shared__ int s_next[EDT_ROWS][M::MAX_CHUNKS];      // the first site after chunk k of the wave's row, -1: none
  const int plane = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * EDT_ROWS + wave;
  const bool live = row < nrows;
  const int base = live ? row * W : 0;
  const int nchunks = (W + 63) / 64;
  int next = -1;
  for (int k = nchunks - 1; k >= 0; --k) {
    if (lane == 0) s_next[wave][k] = next;
    const int w = k * 64 + lane;
    const unsigned long long bal = __ballot(live && w < W && edt_site(src, plane, S, base + w));
    if (bal) next = k * 64 + __builtin_ctzll(bal);
  }
  __syncthreads();
  if (!live) return;
  typename M::T* out = sq + (size_t)plane * S + base;
  int last = -1;
  for (int k = 0; k < nchunks; ++k) {
    const int w = k * 64 + lane;
    const unsigned long long bal = __ballot(w < W && edt_site(src, plane, S, base + w));
    const unsigned long long le = bal & (~0ull >> (63 - lane)), ge = bal & (~0ull << lane);
    const int lpos = le ? k * 64 + 63 - __builtin_clzll(le) : last;
    const int rpos = ge ? k * 64 + __builtin_ctzll(ge) : s_next[wave][k];
    int dist = -1;
    if (lpos >= 0) dist = w - lpos;
    if (rpos >= 0 && (dist < 0 || rpos - w < dist)) dist = rpos - w;
    if (w < W) out[w] = dist < 0 ? M::none() : (typename M::T)M::cost(ww, dist);
    if (bal) last = k * 64 + 63 - __builtin_clzll(bal);
  }
}

// ---- lines ----------------------------------------------------------------------------------------------------------
// Line (o, w) of a plane holds the n voxels o * ostride + i * stride + w.  h pass: o = d, ostride = H W, stride = W,
// n = H; d pass: o = h, ostride = W, stride = H W, n = D.  tw = 1 << ltw lines adjacent along w make the slab of a
// workgroup; dynamic LDS: (n + 2) * tw words.
template <class M>
__global__ __launch_bounds__(EDT_THREADS) void k_edt_lines(typename M::T* __restrict__ sq, int S, int W, int n,
                                                           int stride, int ostride, int ltw, int ntw,
                                                           typename M::Weight wa) {
  using T = typename M::T;
  using Acc = typename M::Acc;
  static_assert(sizeof(T) == sizeof(int), "the slab and the ranges are words");
  extern __shared__ int s_words[];
  const int tw = 1 << ltw, rows = EDT_THREADS >> ltw;
  T* s_g = reinterpret_cast<T*>(s_words);
  int* s_lo = s_words + n * tw;
  int* s_hi = s_lo + tw;
  const int lw = threadIdx.x & (tw - 1), r = threadIdx.x >> ltw;
  const int o = blockIdx.x / ntw, w = (blockIdx.x % ntw) * tw + lw;
  const bool live = w < W;
  T* line = sq + (size_t)blockIdx.y * S + (size_t)o * ostride + (live ? w : 0);
  if (threadIdx.x < tw) {
    s_lo[threadIdx.x] = n;
    s_hi[threadIdx.x] = -1;
  }
  __syncthreads();
  int lo = n, hi = -1;
  for (int i = r; i < n; i += rows) {
    const T g = live ? line[(size_t)i * stride] : M::none();
    s_g[i * tw + lw] = g;
    if (M::finite(g)) {
      lo = min(lo, i);
      hi = i;
    }
  }
  if (hi >= 0) {
    atomicMin(&s_lo[lw], lo);
    atomicMax(&s_hi[lw], hi);
  }
  __syncthreads();
  lo = s_lo[lw];
  hi = s_hi[lw];
  if (!live || hi < 0) return;                         // a line without a finite entry stays as it is
  for (int i = r; i < n; i += rows) {
    Acc best = (Acc)s_g[i * tw + lw];
    for (int j = min(i - 1, hi); j >= lo; --j) {
      const Acc c = M::cost(wa, i - j);
      if (c >= best) break;
      best = M::relax(best, s_g[j * tw + lw], c);
    }
    for (int j = max(i + 1, lo); j <= hi; ++j) {
      const Acc c = M::cost(wa, j - i);
      if (c >= best) break;
      best = M::relax(best, s_g[j * tw + lw], c);
    }
    line[(size_t)i * stride] = (T)best;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
// the limits of effq_edt_sq (include/effq_hip.h): every voxel index and every squared distance fits an int32, and a line
// of the h and d passes fits the LDS of one workgroup
static inline bool edt_dims_ok(int P, int D, int H, int W) {
  return P > 0 && P <= 65535 && D > 0 && H > 0 && W > 0 && (long long)P * D * H * W < (1ll << 31) &&
         (long long)D * D + (long long)H * H + (long long)W * W < (1ll << 31) && D <= EFFQ_EDT_MAX_LINE &&
         H <= EFFQ_EDT_MAX_LINE;
}

template <class M>
static int edt_line_pass(typename M::T* sq, int P, int S, int W, int n, int stride, int nouter, int ostride,
                         typename M::Weight wa, hipStream_t st) {
  if (n == 1) return EFFQ_OK;                          // min over one entry: g + cost(0) = g
  int ltw = 6;
  while (ltw > 0 && (size_t)(n + 2) * sizeof(typename M::T) << ltw > (size_t)EDT_LDS_AIM) --ltw;
  const int tw = 1 << ltw, ntw = (W + tw - 1) / tw;
  const size_t lds = (size_t)(n + 2) * sizeof(typename M::T) << ltw;
  hipLaunchKernelGGL((k_edt_lines<M>), dim3((unsigned)((size_t)nouter * ntw), P), dim3(EDT_THREADS), lds, st, sq, S, W,
                     n, stride, ostride, ltw, ntw, wa);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// the three passes of P planes into sq (P, S): w, then h, then d
template <class M>
static int edt_run(const EdtSrc& src, int P, int D, int H, int W, typename M::Weight wd, typename M::Weight wh,
                   typename M::Weight ww, typename M::T* sq, hipStream_t st) {
  const int S = D * H * W, nrows = D * H;
  hipLaunchKernelGGL((k_edt_rows<M>), dim3((nrows + EDT_ROWS - 1) / EDT_ROWS, P), dim3(EDT_THREADS), 0, st, src, sq, S,
                     W, nrows, ww);
  EFFQ_LAUNCH_CHECK();
  const int rc = edt_line_pass<M>(sq, P, S, W, H, W, D, H * W, wh, st);
  if (rc != EFFQ_OK) return rc;
  return edt_line_pass<M>(sq, P, S, W, D, H * W, H, W, wd, st);
}

}  // namespace effq
