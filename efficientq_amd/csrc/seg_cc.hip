// Connected components of 0/1 volumes and the lesion-level columns of the validation (validate_seg(..., is_cc=True):
// metrics.py:69-94, there three scipy.ndimage.label calls per class on the host).  A block-based union-find:
//
//   masks    (effq_seg_lesions only) decide<MODE, C> of every voxel -> 16 decision bits per voxel, pred | gt << 8
//   tiles    every tile of 8 x 8 x 32 voxels is labelled in LDS: a voxel starts at the first voxel of its run along w
//            (one ballot per row, no atomics), runs of adjacent rows are joined by an atomicMin union in LDS, and each
//            voxel is written out as 1 + the volume index of its tile-local root
//   merge    the voxels on a tile surface join their component to the neighbours' in the adjacent tiles (faces, and for
//            26-connectivity edges and corners) by the same union on the global label array
//   flatten  every voxel is pointed at its root; a voxel that both masks of a class hold flags the two roots
//   count    roots and roots without a flag, per-block partials, added in block order by the last launch
//
// cc_run, the launches after the masks, also serves the lesion table (seg_cc_table.hip) and the rules of --post
// (label_post.hip) through seg_cc.h.
//
// The parent of a voxel always has a smaller index than the voxel, so the root of a component is its least index whatever
// order the unions ran in: the labels are the same bits every time.  Every loop ends by itself: a find walks down strictly
// decreasing indices to a root, and a union that loses its atomicMin goes on from the smaller value the atomic returned.
// No workgroup waits for another.  A find may read a value that another compute die has meanwhile lowered: the stale value
// is an older parent in the same component, and only the value an atomicMin returns decides that a union is done.
#include "common.h"
#include "seg_decide.h"
#include "seg_cc.h"

namespace effq {

constexpr int CC_TD = 8, CC_TH = 8, CC_TW = 32;        // tile: 2048 voxels, 8 KB of LDS, rows of 128 B of labels
constexpr int CC_TVOX = CC_TD * CC_TH * CC_TW;
constexpr int CC_VPT = CC_TVOX / CC_THREADS;
static_assert(CC_TW == 32 && CC_THREADS % 64 == 0, "one ballot holds two rows of a tile");

__device__ __forceinline__ bool cc_fg(const CcSrc& s, int plane, int S, int idx) {
  if (s.bits) return (s.bits[idx] >> (plane < s.C ? plane : 8 + plane - s.C)) & 1;
  return s.masks[(size_t)plane * S + idx] != 0;
}

// ---- union-find -----------------------------------------------------------------------------------------------------
// LDS: L[i] = parent of tile voxel i (itself for a root), -1 for background
__device__ __forceinline__ int lds_find(const int* L, int i) {
  for (;;) {
    const int p = __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == i) return i;
    i = p;
  }
}

__device__ __forceinline__ void lds_union(int* L, int a, int b) {
  for (;;) {
    a = lds_find(L, a);
    b = lds_find(L, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[b], a);
    if (old == b) return;       // b was a root and now hangs under a
    b = old;                    // somebody lowered it first: go on from there (old < b)
  }
}

// global: L[i] = 1 + parent of voxel i (1 + i for a root), 0 for background
__device__ __forceinline__ int cc_find(const int* L, int i) {
  for (;;) {
    const int p = __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
    if (p == i) return i;
    i = p;
  }
}

__device__ __forceinline__ void cc_union(int* L, int a, int b) {
  for (;;) {
    a = cc_find(L, a);
    b = cc_find(L, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[b], a + 1) - 1;
    if (old == b) return;
    b = old;
  }
}

// the rows that hold the neighbours of smaller index: (dz, dy); each pair of neighbours is looked at from its larger voxel
template <int CONN>
struct CcRows;
template <>
struct CcRows<26> {
  static constexpr int N = 4;
  static constexpr int DZ[4] = {-1, -1, -1, 0};
  static constexpr int DY[4] = {-1, 0, 1, -1};
};
template <>
struct CcRows<6> {
  static constexpr int N = 2;
  static constexpr int DZ[2] = {-1, 0};
  static constexpr int DY[2] = {0, -1};
};

// ---- tiles ----------------------------------------------------------------------------------------------------------
// Which unions are made (here and in k_cc_merge): a voxel joins the voxel straight across in an adjacent row unless its
// left neighbour does the same one step to the left (both runs go on to the left, the pair there joins them); when the
// voxel straight across is background it joins the two diagonal ones (26 only), the left one unless the voxel's own left
// neighbour is foreground and sees it straight across.  A skipped pair is always joined through pairs further left.
template <int CONN>
__global__ __launch_bounds__(CC_THREADS) void k_cc_tiles(CcSrc src, int* __restrict__ labels, int D, int H, int W,
                                                         int nth, int ntw) {
  __shared__ int L[CC_TVOX];
  using R = CcRows<CONN>;
  const int plane = blockIdx.y;
  const int S = D * H * W;
  int t = blockIdx.x;
  const int w0 = (t % ntw) * CC_TW; t /= ntw;
  const int h0 = (t % nth) * CC_TH;
  const int d0 = (t / nth) * CC_TD;
  int* out = labels + (size_t)plane * S;

  // a voxel starts at the first voxel of its run along w: the ballot holds two rows of 32
#pragma unroll
  for (int k = 0; k < CC_VPT; ++k) {
    const int i = threadIdx.x + CC_THREADS * k;
    const int lw = i & 31, lh = (i >> 5) & 7, ld = i >> 8;
    const int d = d0 + ld, h = h0 + lh, w = w0 + lw;
    const bool fg = d < D && h < H && w < W && cc_fg(src, plane, S, (d * H + h) * W + w);
    const unsigned long long bal = __ballot(fg);
    const uint32_t row = (uint32_t)(bal >> (threadIdx.x & 32));
    const uint32_t below = ~row & ((1u << lw) - 1u);            // background to the left of this voxel in its row
    const int start = below ? 32 - __clz(below) : 0;
    L[i] = fg ? i - lw + start : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CC_VPT; ++k) {
    const int i = threadIdx.x + CC_THREADS * k;
    if (L[i] < 0) continue;
    const int lw = i & 31, lh = (i >> 5) & 7, ld = i >> 8;
    const bool left = lw > 0 && L[i - 1] >= 0;
#pragma unroll
    for (int r = 0; r < R::N; ++r) {
      const int nd = ld + R::DZ[r], nh = lh + R::DY[r];
      if (nd < 0 || nh < 0 || nh >= CC_TH) continue;
      const int n0 = (nd * CC_TH + nh) * CC_TW + lw;
      if (L[n0] >= 0) {
        if (!(left && L[n0 - 1] >= 0)) lds_union(L, i, n0);
      } else if constexpr (CONN == 26) {
        if (lw > 0 && !left && L[n0 - 1] >= 0) lds_union(L, i, n0 - 1);
        if (lw < CC_TW - 1 && L[n0 + 1] >= 0) lds_union(L, i, n0 + 1);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CC_VPT; ++k) {
    const int i = threadIdx.x + CC_THREADS * k;
    const int lw = i & 31, lh = (i >> 5) & 7, ld = i >> 8;
    const int d = d0 + ld, h = h0 + lh, w = w0 + lw;
    if (d >= D || h >= H || w >= W) continue;
    int l = 0;
    if (L[i] >= 0) {
      const int r = lds_find(L, i);
      l = 1 + ((d0 + (r >> 8)) * H + h0 + ((r >> 5) & 7)) * W + w0 + (r & 31);
    }
    out[(d * H + h) * W + w] = l;
  }
}

// ---- merge ----------------------------------------------------------------------------------------------------------
template <int CONN>
__global__ __launch_bounds__(CC_THREADS) void k_cc_merge(int* __restrict__ labels, int D, int H, int W) {
  using R = CcRows<CONN>;
  const int S = D * H * W;
  int* L = labels + (size_t)blockIdx.y * S;
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)i;
    const int w = v % W, q = v / W, h = q % H, d = q / H;
    const int ld = d & (CC_TD - 1), lh = h & (CC_TH - 1), lw = w & (CC_TW - 1);
    // only a voxel on the surface of its tile has a neighbour of smaller index in another tile
    if (ld != 0 && lh != 0 && lw != 0 && (CONN == 6 || (lh != CC_TH - 1 && lw != CC_TW - 1))) continue;
    if (L[v] == 0) continue;
    const bool left = w > 0 && L[v - 1] != 0;
    if (lw == 0 && left) cc_union(L, v, v - 1);
#pragma unroll
    for (int r = 0; r < R::N; ++r) {
      const int nd = d + R::DZ[r], nh = h + R::DY[r];
      if (nd < 0 || nh < 0 || nh >= H) continue;
      // the whole row lies in another tile, or only its ends can
      const bool rowcross = (R::DZ[r] < 0 && ld == 0) || (R::DY[r] < 0 && lh == 0) || (R::DY[r] > 0 && lh == CC_TH - 1);
      if (!rowcross && (CONN == 6 || (lw != 0 && lw != CC_TW - 1))) continue;
      const int n0 = (nd * H + nh) * W + w;
      if (L[n0] != 0) {
        if (rowcross && !(left && L[n0 - 1] != 0)) cc_union(L, v, n0);
      } else if constexpr (CONN == 26) {
        if (w > 0 && !left && (rowcross || lw == 0) && L[n0 - 1] != 0) cc_union(L, v, n0 - 1);
        if (w < W - 1 && (rowcross || lw == CC_TW - 1) && L[n0 + 1] != 0) cc_union(L, v, n0 + 1);
      }
    }
  }
}

// ---- flatten --------------------------------------------------------------------------------------------------------
// bits / flags null: labels only.  Plane q < C is the predicted mask of class q, plane C + q its label mask: a voxel that
// both hold flags its root in both planes (plain stores of 1; the flags were zeroed before).
__global__ __launch_bounds__(CC_THREADS) void k_cc_flatten(int* __restrict__ labels, const uint16_t* __restrict__ bits,
                                                           uint8_t* __restrict__ flags, int C, int S) {
  const int plane = blockIdx.y;
  int* L = labels + (size_t)plane * S;
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)i;
    if (L[v] == 0) continue;
    const int r = cc_find(L, v);
    L[v] = r + 1;
    if (flags) {
      const int c = plane < C ? plane : plane - C;
      const uint32_t b = bits[v];
      if ((b >> c) & (b >> (8 + c)) & 1u) flags[(size_t)plane * S + r] = 1;
    }
  }
}

// ---- count ----------------------------------------------------------------------------------------------------------
// partial (P, gridDim.x, 2): roots of the plane, and roots without a flag (flags null: 0)
__global__ __launch_bounds__(CC_THREADS) void k_cc_count(const int* __restrict__ labels,
                                                         const uint8_t* __restrict__ flags, int S,
                                                         uint32_t* __restrict__ partial) {
  const int plane = blockIdx.y;
  const int* L = labels + (size_t)plane * S;
  uint32_t roots = 0, bare = 0;
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)i;
    if (L[v] != v + 1) continue;
    ++roots;
    if (flags && flags[(size_t)plane * S + v] == 0) ++bare;
  }
  __shared__ uint32_t red[CC_WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  roots = wave_sum_all(roots);
  bare = wave_sum_all(bare);
  if (lane == 0) {
    red[wave][0] = roots;
    red[wave][1] = bare;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    uint32_t s = 0;
    for (int w = 0; w < CC_WAVES; ++w) s += red[w][threadIdx.x];
    partial[((size_t)plane * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = s;
  }
}

// one thread per plane adds its partials in block order.  C == 0: out (P) = components.  Else out (C, 4) = totall, predl,
// fnl, fpl from the planes c (predicted) and C + c (label).
__global__ __launch_bounds__(64) void k_cc_final(const uint32_t* __restrict__ partial, int nblocks, int P, int C,
                                                 long long* __restrict__ out) {
  const int plane = blockIdx.x * 64 + threadIdx.x;
  if (plane >= P) return;
  long long roots = 0, bare = 0;
  for (int b = 0; b < nblocks; ++b) {
    roots += partial[((size_t)plane * nblocks + b) * 2];
    bare += partial[((size_t)plane * nblocks + b) * 2 + 1];
  }
  if (C == 0) {
    out[plane] = roots;
  } else if (plane < C) {
    out[4 * plane + 1] = roots;
    out[4 * plane + 3] = bare;
  } else {
    out[4 * (plane - C) + 0] = roots;
    out[4 * (plane - C) + 2] = bare;
  }
}

// the launches after the masks; C == 0: plain labelling (no flags), out = ncomp (P)
int cc_run(const CcSrc& src, int P, int D, int H, int W, int conn, int* labels, uint8_t* flags, int C, uint32_t* partial,
           long long* out, hipStream_t st) {
  const int S = D * H * W;
  const int ntd = (D + CC_TD - 1) / CC_TD, nth = (H + CC_TH - 1) / CC_TH, ntw = (W + CC_TW - 1) / CC_TW;
  const dim3 b(CC_THREADS);
  const dim3 gt((unsigned)((size_t)ntd * nth * ntw), P), gs(cc_grid(S, CC_STREAM_BLOCKS), P);
  const unsigned nb = cc_grid(S, CC_COUNT_BLOCKS);
  if (flags) EFFQ_HIP(hipMemsetAsync(flags, 0, (size_t)P * S, st));
  if (conn == 26) hipLaunchKernelGGL(k_cc_tiles<26>, gt, b, 0, st, src, labels, D, H, W, nth, ntw);
  else hipLaunchKernelGGL(k_cc_tiles<6>, gt, b, 0, st, src, labels, D, H, W, nth, ntw);
  EFFQ_LAUNCH_CHECK();
  if (conn == 26) hipLaunchKernelGGL(k_cc_merge<26>, gs, b, 0, st, labels, D, H, W);
  else hipLaunchKernelGGL(k_cc_merge<6>, gs, b, 0, st, labels, D, H, W);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_flatten, gs, b, 0, st, labels, src.bits, flags, C, S);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_count, dim3(nb, P), b, 0, st, labels, flags, S, partial);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_final, dim3((P + 63) / 64), dim3(64), 0, st, partial, (int)nb, P, C, out);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // namespace effq
using namespace effq;

extern "C" {

size_t effq_cc_ws_bytes(int P, int D, int H, int W) {
  if (!cc_dims_ok(P, D, H, W)) return 0;
  return cc_ws(nullptr, P, (size_t)D * H * W).bytes;
}

int effq_cc_label(const uint8_t* masks, int P, int D, int H, int W, int connectivity, int32_t* labels,
                  long long* ncomp, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(masks && labels && ncomp && ws);
  EFFQ_CHECK_ARG(cc_dims_ok(P, D, H, W));
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  const CcWs s = cc_ws(ws, P, (size_t)D * H * W);
  EFFQ_CHECK_WS(ws_bytes, s.bytes);
  return cc_run(cc_src_masks(masks), P, D, H, W, connectivity, labels, nullptr, 0, s.partial, ncomp, as_stream(stream));
}

int effq_seg_lesions(const float* logits, const uint8_t* label, int C, int D, int H, int W, int mode, int fuse,
                     float thresh, int connectivity, long long* counts, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(logits && label && counts && ws && C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(cc_dims_ok(2 * C, D, H, W));
  EFFQ_CHECK_ARG(mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID);
  EFFQ_CHECK_ARG(fuse == EFFQ_SEG_FUSE_NONE || fuse == EFFQ_SEG_FUSE_AGG || fuse == EFFQ_SEG_FUSE_CON);
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  const int P = 2 * C;
  const size_t S = (size_t)D * H * W;
  const CcWs s = cc_ws(ws, P, S);
  EFFQ_CHECK_WS(ws_bytes, s.bytes);
  const hipStream_t st = as_stream(stream);
  const int rc = cc_decision_bits(logits, label, C, S, mode, fuse, thresh, s.bits, st);
  if (rc != EFFQ_OK) return rc;
  return cc_run(cc_src_bits(s.bits, C), P, D, H, W, connectivity, s.labels, s.flags, C, s.partial, counts, st);
}

}  // extern "C"
