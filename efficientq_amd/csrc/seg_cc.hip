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
//   table    (effq_cc_table, effq_seg_lesion_table) one record per component, four more launches: see "table" below
//   clean    (effq_label_clean) the components of a label map's values sized at their roots and the small or losing ones
//            relabelled: see "clean" below
//   post     (effq_label_post) the same rules, and holes filled and masks closed or opened by a ball, the latter through
//            the distance transform of seg_surf.h: see "post" below
//
// The parent of a voxel always has a smaller index than the voxel, so the root of a component is its least index whatever
// order the unions ran in: the labels are the same bits every time.  Every loop ends by itself: a find walks down strictly
// decreasing indices to a root, and a union that loses its atomicMin goes on from the smaller value the atomic returned.
// No workgroup waits for another.  A find may read a value that another compute die has meanwhile lowered: the stale value
// is an older parent in the same component, and only the value an atomicMin returns decides that a union is done.
#include "common.h"
#include "seg_decide.h"
#include "seg_masks.h"
#include "seg_surf.h"

namespace effq {

constexpr int CC_TD = 8, CC_TH = 8, CC_TW = 32;        // tile: 2048 voxels, 8 KB of LDS, rows of 128 B of labels
constexpr int CC_TVOX = CC_TD * CC_TH * CC_TW;
constexpr int CC_VPT = CC_TVOX / CC_THREADS;
constexpr int CC_WAVES = CC_THREADS / 64;
constexpr int CC_COUNT_BLOCKS = 512;                   // count: blocks per plane at most = partials per plane
static_assert(CC_TW == 32 && CC_THREADS % 64 == 0, "one ballot holds two rows of a tile");

// where the foreground of plane q comes from: P masks of uint8, or bit q of the decision bits (pred | gt << 8)
struct CcSrc {
  const uint8_t* masks;
  const uint16_t* bits;
  int C;
};

__device__ __forceinline__ bool cc_fg(const CcSrc& s, int plane, int S, int idx) {
  if (s.bits) return (s.bits[idx] >> (plane < s.C ? plane : 8 + plane - s.C)) & 1;
  return s.masks[(size_t)plane * S + idx] != 0;
}

static inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

struct CcWs {
  uint32_t* partial;   // (P, CC_COUNT_BLOCKS, 2)
  int* labels;         // (P, S)
  uint16_t* bits;      // (S)
  uint8_t* flags;      // (P, S)
  size_t bytes;
};

static CcWs cc_ws(void* ws, int P, size_t S) {
  CcWs r;
  char* p = static_cast<char*>(ws);
  size_t off = 0;
  r.partial = reinterpret_cast<uint32_t*>(p + off); off += align16((size_t)P * CC_COUNT_BLOCKS * 2 * sizeof(uint32_t));
  r.labels = reinterpret_cast<int*>(p + off);       off += align16((size_t)P * S * sizeof(int));
  r.bits = reinterpret_cast<uint16_t*>(p + off);    off += align16(S * sizeof(uint16_t));
  r.flags = reinterpret_cast<uint8_t*>(p + off);    off += align16((size_t)P * S);
  r.bytes = off;
  return r;
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
__device__ __forceinline__ uint32_t cc_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

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
  roots = cc_wave_sum(roots);
  bare = cc_wave_sum(bare);
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
static int cc_run(const CcSrc& src, int P, int D, int H, int W, int conn, int* labels, uint8_t* flags, int C,
                  uint32_t* partial, long long* out, hipStream_t st) {
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

static bool cc_dims_ok(int P, int D, int H, int W) {
  return P > 0 && P <= 65535 && D > 0 && H > 0 && W > 0 && (long long)P * D * H * W < (1ll << 31);
}

// ---- table ----------------------------------------------------------------------------------------------------------
// One row per component, in ascending order of its first voxel (scipy.ndimage.label's numbering), from the flattened
// labels of cc_run (labels[v] = root + 1, a root has labels[v] == v + 1):
//
//   chunks   the roots of every chunk of CC_CHUNK consecutive voxels are counted (ballots, no atomics)
//   scan     one workgroup per plane: exclusive scan of the chunk counts in place, the total is nrows
//   rank     every chunk is walked again: the k-th root of the plane gets row k = {first voxel, 0, 0} (k < max_rows) and
//            its own label word becomes -(k + 1), so a voxel finds its row through labels[labels[v] - 1]
//   accum    every foreground voxel adds 1 to the size of its row, and 1 to its overlap when both masks of its class
//            hold the voxel: equal rows of a wave are added once (the lane count), the sums of a workgroup are kept in
//            LDS slots and reach the table once per slot
//
// Integer adds only: equal inputs give equal bits.  A workgroup reads and writes the label words of its own chunk only
// (rank), and the accumulation runs in a launch of its own after it.
constexpr int CC_CHUNK = EFFQ_CC_TABLE_CHUNK;
constexpr int CC_CHUNK_ITERS = CC_CHUNK / CC_THREADS;  // ballots per wave: a wave owns CC_CHUNK / CC_WAVES voxels in a row
constexpr int CC_SLOTS = 256;                          // accum: rows a workgroup keeps in LDS (direct-mapped)
constexpr int CC_MATCH_ROUNDS = 4;                     // accum: distinct rows of a wave that are combined by ballot
static_assert(CC_CHUNK % CC_THREADS == 0, "a chunk is a whole number of ballots per wave");

struct CcTableWs {
  CcWs cc;
  uint32_t* chunks;    // (P, nchunks)
  int nchunks;
  size_t bytes;
};

static CcTableWs cc_table_ws(void* ws, int P, size_t S) {
  CcTableWs r;
  r.cc = cc_ws(ws, P, S);
  r.nchunks = (int)((S + CC_CHUNK - 1) / CC_CHUNK);
  r.chunks = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + r.cc.bytes);
  r.bytes = r.cc.bytes + align16((size_t)P * r.nchunks * sizeof(uint32_t));
  return r;
}

// WRITE false: chunks (P, gridDim.x) = the roots of each chunk.  WRITE true: chunks holds the exclusive scan; the roots
// get their rows and their negative label words.  rows (P, max_rows, stride) int32.
template <bool WRITE>
__global__ __launch_bounds__(CC_THREADS) void k_cc_rank(int* __restrict__ labels, int S, uint32_t* __restrict__ chunks,
                                                        int max_rows, int stride, int32_t* __restrict__ rows) {
  __shared__ uint32_t s_wave[CC_WAVES];
  const int plane = blockIdx.y;
  int* L = labels + (size_t)plane * S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * CC_CHUNK + (long long)wave * (CC_CHUNK / CC_WAVES);
  unsigned long long bal[CC_CHUNK_ITERS];
  uint32_t n = 0;
#pragma unroll
  for (int k = 0; k < CC_CHUNK_ITERS; ++k) {
    const long long v = base + k * 64 + lane;
    bal[k] = __ballot(v < S && L[v] == (int)v + 1);
    n += (uint32_t)__popcll(bal[k]);
  }
  if (lane == 0) s_wave[wave] = n;
  __syncthreads();
  const size_t slot = (size_t)plane * gridDim.x + blockIdx.x;
  if constexpr (!WRITE) {
    if (threadIdx.x == 0) {
      uint32_t s = 0;
      for (int w = 0; w < CC_WAVES; ++w) s += s_wave[w];
      chunks[slot] = s;
    }
  } else {
    uint32_t off = chunks[slot];
    for (int w = 0; w < wave; ++w) off += s_wave[w];
#pragma unroll
    for (int k = 0; k < CC_CHUNK_ITERS; ++k) {
      if ((bal[k] >> lane) & 1ull) {
        const int v = (int)(base + k * 64 + lane);
        const uint32_t r = off + (uint32_t)__popcll(bal[k] & ((1ull << lane) - 1ull));
        L[v] = -(int)r - 1;
        if (r < (uint32_t)max_rows) {
          int32_t* row = rows + ((size_t)plane * max_rows + r) * stride;
          row[0] = v;
          for (int j = 1; j < stride; ++j) row[j] = 0;
        }
      }
      off += (uint32_t)__popcll(bal[k]);
    }
  }
}

// one workgroup per plane: thread t owns a run of consecutive chunks, the runs are scanned in LDS
__global__ __launch_bounds__(CC_THREADS) void k_cc_scan(uint32_t* __restrict__ chunks, int nchunks,
                                                        long long* __restrict__ nrows) {
  __shared__ uint32_t s_sum[CC_THREADS];
  uint32_t* c = chunks + (size_t)blockIdx.x * nchunks;
  const int t = threadIdx.x;
  const int per = (nchunks + CC_THREADS - 1) / CC_THREADS;
  const int b0 = min(nchunks, t * per), b1 = min(nchunks, b0 + per);
  uint32_t sum = 0;
  for (int b = b0; b < b1; ++b) sum += c[b];
  s_sum[t] = sum;
  __syncthreads();
  for (int o = 1; o < CC_THREADS; o <<= 1) {
    const uint32_t add = t >= o ? s_sum[t - o] : 0u;
    __syncthreads();
    s_sum[t] += add;
    __syncthreads();
  }
  uint32_t run = s_sum[t] - sum;          // exclusive
  for (int b = b0; b < b1; ++b) {
    const uint32_t k = c[b];
    c[b] = run;
    run += k;
  }
  if (t == CC_THREADS - 1) nrows[blockIdx.x] = (long long)s_sum[t];
}

// bits null: sizes only (stride 2).  Else plane q < C is the predicted mask of class q, plane C + q its label mask, and
// row[2] counts the voxels that both hold.
__global__ __launch_bounds__(CC_THREADS) void k_cc_accum(const int* __restrict__ labels,
                                                         const uint16_t* __restrict__ bits, int C, int S, int max_rows,
                                                         int stride, int32_t* __restrict__ rows) {
  __shared__ int s_key[CC_SLOTS];
  __shared__ uint32_t s_size[CC_SLOTS], s_ovl[CC_SLOTS];
  const int plane = blockIdx.y;
  const int* L = labels + (size_t)plane * S;
  int32_t* T = rows + (size_t)plane * max_rows * stride;
  const int c = plane < C ? plane : plane - C;
  for (int k = threadIdx.x; k < CC_SLOTS; k += CC_THREADS) {
    s_key[k] = -1;
    s_size[k] = 0;
    s_ovl[k] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  // the trip count is the same for every lane of a wave: the ballots below need them all
  for (long long i0 = (long long)blockIdx.x * CC_THREADS; i0 < S; i0 += (long long)gridDim.x * CC_THREADS) {
    const long long i = i0 + threadIdx.x;
    int r = -1;                            // the row of this lane's voxel; -1: nothing to add
    bool both = false;
    if (i < S) {
      const int l = L[i];
      if (l != 0) {
        r = l < 0 ? -l - 1 : -L[l - 1] - 1;
        if (r >= max_rows) r = -1;
        if (bits && r >= 0) {
          const uint32_t b = bits[i];
          both = ((b >> c) & (b >> (8 + c)) & 1u) != 0;
        }
      }
    }
    unsigned long long todo = __ballot(r >= 0);
    uint32_t dsize = 0, dovl = 0;          // what this lane adds: the leader of a group carries the group's counts
    for (int round = 0; round < CC_MATCH_ROUNDS && todo; ++round) {
      const int lead = __ffsll((long long)todo) - 1;
      const int key = __shfl(r, lead, 64);
      const unsigned long long m = __ballot(r == key) & todo;
      const unsigned long long mo = __ballot(r == key && both) & todo;
      if (lane == lead) {
        dsize = (uint32_t)__popcll(m);
        dovl = (uint32_t)__popcll(mo);
      }
      todo &= ~m;
    }
    if ((todo >> lane) & 1ull) {           // more distinct rows than rounds: one add per voxel
      dsize = 1;
      dovl = both ? 1u : 0u;
    }
    if (dsize == 0) continue;
    const int s = r & (CC_SLOTS - 1);
    int k = s_key[s];
    if (k == -1) {
      k = atomicCAS(&s_key[s], -1, r);
      if (k == -1) k = r;
    }
    if (k == r) {
      atomicAdd(&s_size[s], dsize);
      if (dovl) atomicAdd(&s_ovl[s], dovl);
    } else {                               // the slot belongs to another row
      atomicAdd(&T[(size_t)r * stride + 1], (int)dsize);
      if (dovl) atomicAdd(&T[(size_t)r * stride + 2], (int)dovl);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < CC_SLOTS; k += CC_THREADS) {
    const int r = s_key[k];
    if (r < 0) continue;
    atomicAdd(&T[(size_t)r * stride + 1], (int)s_size[k]);
    if (s_ovl[k]) atomicAdd(&T[(size_t)r * stride + 2], (int)s_ovl[k]);
  }
}

// the four launches after cc_run; bits null: sizes only
static int cc_table_run(const CcTableWs& t, const uint16_t* bits, int C, int P, int S, int max_rows, int stride,
                        int32_t* rows, long long* nrows, hipStream_t st) {
  const dim3 b(CC_THREADS), gc(t.nchunks, P);
  hipLaunchKernelGGL(k_cc_rank<false>, gc, b, 0, st, t.cc.labels, S, t.chunks, max_rows, stride, rows);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_scan, dim3(P), b, 0, st, t.chunks, t.nchunks, nrows);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_rank<true>, gc, b, 0, st, t.cc.labels, S, t.chunks, max_rows, stride, rows);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_accum, dim3(cc_grid(S, CC_STREAM_BLOCKS), P), b, 0, st, t.cc.labels, bits, C, S, max_rows,
                     stride, rows);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// ---- clean ----------------------------------------------------------------------------------------------------------
// effq_label_clean: the rules of --post on a uint8 label map, one after the other on the map the previous rule left.  Per
// rule, after the five launches of cc_run on the plane "the voxel's value is in the rule's set":
//
//   mask     (before cc_run) the membership of every voxel -> one 0/1 plane; the size words are zeroed in the same pass
//   sizes    every foreground voxel adds 1 to the size word of its root: equal roots of a wave are added once (the lane
//            count), as k_cc_accum does
//   best     (largest only) every root offers size << 32 | (0xFFFFFFFF - root) to one 64-bit atomicMax: the largest size
//            wins, and of equal sizes the least root (the component whose first voxel comes first)
//   apply    the voxels of a losing (largest) or small (min) component become TO and are counted
//
// Integer adds and one max only: equal inputs give equal bits.  The map is rewritten in place (`out`, a copy of `in` when
// they differ): a voxel is written by the thread that read it, and the labels of a rule are complete before its apply.
struct CleanSet {
  unsigned long long w[4];   // bit v set: the value v is in the rule's mask
};

struct CleanWs {
  uint32_t* partial;             // (CC_COUNT_BLOCKS, 2): cc_run's
  int* labels;                   // (S)
  int* sizes;                    // (S): the voxels of a component, at its root
  uint8_t* mask;                 // (S)
  unsigned long long* best;      // (EFFQ_LABEL_CLEAN_MAX_RULES)
  size_t bytes;
};

static CleanWs clean_ws(void* ws, size_t S) {
  CleanWs r;
  char* p = static_cast<char*>(ws);
  size_t off = 0;
  r.partial = reinterpret_cast<uint32_t*>(p + off); off += align16((size_t)CC_COUNT_BLOCKS * 2 * sizeof(uint32_t));
  r.labels = reinterpret_cast<int*>(p + off);       off += align16(S * sizeof(int));
  r.sizes = reinterpret_cast<int*>(p + off);        off += align16(S * sizeof(int));
  r.mask = reinterpret_cast<uint8_t*>(p + off);     off += align16(S);
  r.best = reinterpret_cast<unsigned long long*>(p + off);
  off += align16(EFFQ_LABEL_CLEAN_MAX_RULES * sizeof(unsigned long long));
  r.bytes = off;
  return r;
}

// stats (R, 2) and best (R) start at 0: the relabelled voxels and the counts of effq_label_post's rules are added to;
// the components of a largest / min rule are written over the first word by k_cc_final
__global__ __launch_bounds__(64) void k_clean_init(unsigned long long* __restrict__ best, long long* __restrict__ stats,
                                                   int R) {
  const int r = threadIdx.x;
  if (r >= R) return;
  best[r] = 0ull;
  stats[2 * r] = 0;
  stats[2 * r + 1] = 0;
}

__global__ __launch_bounds__(CC_THREADS) void k_clean_mask(const uint8_t* __restrict__ map, CleanSet set, int S,
                                                           uint8_t* __restrict__ mask, int* __restrict__ sizes) {
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const uint32_t v = map[i];
    mask[i] = (uint8_t)((set.w[v >> 6] >> (v & 63u)) & 1ull);
    sizes[i] = 0;
  }
}

// labels: flattened (labels[v] = root + 1, 0 for background)
__global__ __launch_bounds__(CC_THREADS) void k_clean_sizes(const int* __restrict__ labels, int S,
                                                            int* __restrict__ sizes) {
  const int lane = threadIdx.x & 63;
  // the trip count is the same for every lane of a wave: the ballots below need them all
  for (long long i0 = (long long)blockIdx.x * CC_THREADS; i0 < S; i0 += (long long)gridDim.x * CC_THREADS) {
    const long long i = i0 + threadIdx.x;
    const int r = i < S ? labels[i] - 1 : -1;      // the root of this lane's voxel; -1: nothing to add
    unsigned long long todo = __ballot(r >= 0);
    int add = 0;                                    // the leader of a group carries the group's count
    for (int round = 0; round < CC_MATCH_ROUNDS && todo; ++round) {
      const int lead = __ffsll((long long)todo) - 1;
      const int key = __shfl(r, lead, 64);
      const unsigned long long m = __ballot(r == key) & todo;
      if (lane == lead) add = __popcll(m);
      todo &= ~m;
    }
    if ((todo >> lane) & 1ull) add = 1;            // more distinct roots than rounds: one add per voxel
    if (add) atomicAdd(&sizes[r], add);
  }
}

__global__ __launch_bounds__(CC_THREADS) void k_clean_best(const int* __restrict__ labels,
                                                           const int* __restrict__ sizes, int S,
                                                           unsigned long long* __restrict__ best) {
  unsigned long long key = 0ull;
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)i;
    if (labels[v] != v + 1) continue;
    const unsigned long long k = ((unsigned long long)(uint32_t)sizes[v] << 32) | (0xFFFFFFFFull - (uint32_t)v);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0 && key) atomicMax(best, key);
}

// OP LARGEST: every component but the winner of `best` loses; OP MIN: every component of fewer than n voxels does
template <int OP>
__global__ __launch_bounds__(CC_THREADS) void k_clean_apply(const int* __restrict__ labels,
                                                            const int* __restrict__ sizes,
                                                            const unsigned long long* __restrict__ best, long long n,
                                                            int to, int S, uint8_t* __restrict__ map,
                                                            unsigned long long* __restrict__ changed) {
  int keep = -1;
  if constexpr (OP == EFFQ_LABEL_CLEAN_LARGEST) keep = (int)(0xFFFFFFFFu - (uint32_t)(*best & 0xFFFFFFFFull));
  uint32_t cnt = 0;
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const int l = labels[i];
    if (l == 0) continue;
    const bool lose = OP == EFFQ_LABEL_CLEAN_LARGEST ? l - 1 != keep : (long long)sizes[l - 1] < n;
    if (lose) {
      map[i] = (uint8_t)to;
      ++cnt;
    }
  }
  __shared__ uint32_t red[CC_WAVES];
  cnt = cc_wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < CC_WAVES; ++w) s += red[w];
    if (s) atomicAdd(changed, (unsigned long long)s);
  }
}

// one rule of effq_label_clean on the map `out`: 8 launches for MIN, 9 for LARGEST.  rule = op, N, TO (checked);
// stats (2) = components (written by k_cc_final), relabelled voxels (added to); best: the rule's word, zero before
static int clean_rule_run(const CleanWs& s, const CleanSet& set, const long long* rule, int D, int H, int W,
                          int connectivity, uint8_t* out, long long* stats, unsigned long long* best, hipStream_t st) {
  const int S = D * H * W;
  const dim3 b(CC_THREADS), gs(cc_grid((size_t)S, CC_STREAM_BLOCKS));
  const long long n = rule[1];
  const int to = (int)rule[2];
  unsigned long long* changed = reinterpret_cast<unsigned long long*>(stats + 1);
  CcSrc src;
  src.masks = s.mask; src.bits = nullptr; src.C = 0;
  hipLaunchKernelGGL(k_clean_mask, gs, b, 0, st, out, set, S, s.mask, s.sizes);
  EFFQ_LAUNCH_CHECK();
  const int rc = cc_run(src, 1, D, H, W, connectivity, s.labels, nullptr, 0, s.partial, stats, st);
  if (rc != EFFQ_OK) return rc;
  hipLaunchKernelGGL(k_clean_sizes, gs, b, 0, st, s.labels, S, s.sizes);
  EFFQ_LAUNCH_CHECK();
  if (rule[0] == EFFQ_LABEL_CLEAN_LARGEST) {
    hipLaunchKernelGGL(k_clean_best, gs, b, 0, st, s.labels, s.sizes, S, best);
    EFFQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_clean_apply<EFFQ_LABEL_CLEAN_LARGEST>, gs, b, 0, st, s.labels, s.sizes, best, n, to, S, out,
                       changed);
  } else {
    hipLaunchKernelGGL(k_clean_apply<EFFQ_LABEL_CLEAN_MIN>, gs, b, 0, st, s.labels, s.sizes, best, n, to, S, out,
                       changed);
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// ---- post -----------------------------------------------------------------------------------------------------------
// effq_label_post: the rules of effq_label_clean (clean_rule_run above, the same launches) and three morphological ones,
// on the mask M = "the voxel's value is in the rule's set" of the map the previous rule left.
//
//   fill     the complement of M is labelled at the dual connectivity (cc_run), every complement voxel on a face of the
//            volume marks its root (plain stores of 1), and the voxels of the unmarked components - the holes - become TO
//            and are counted, the roots among them as holes: 8 launches
//   close    M is written into a plane padded by R background voxels on every side, the exact distance transform of
//            seg_surf.h runs on it, a threshold writes the complement of the dilation {sq <= R^2} as the sites of a second
//            transform, and the voxels outside M whose second distance exceeds R^2 - the erosion of the dilation - become
//            TO: a memset and 9 launches
//   open     the same skeleton from the complement of M with the pad as sites: the first threshold is the erosion, the
//            voxels of M further than R from it become TO
//
// The pad makes both transforms those of the infinite grid with background outside the volume: a voxel outside the padded
// plane is more than R away from every voxel of the volume.  A plane without sites is INT32_MAX throughout, which the
// thresholds read as "further than R".  Integer compares and adds only: equal inputs give equal bits.
struct PostWs {
  CleanWs clean;                 // first: with max_radius 0 the workspace is effq_label_clean's and the words below
  long long* ncomp;              // (2): cc_run's component count of a fill rule (not reported)
  uint8_t* site;                 // (Sp): the sites of the padded plane
  int* sq;                       // (Sp): its squared distances
  size_t bytes;
};

static bool post_dims_ok(int D, int H, int W, int max_radius) {
  if (!cc_dims_ok(1, D, H, W) || max_radius < 0 || max_radius > EFFQ_LABEL_POST_MAX_RADIUS) return false;
  if (max_radius == 0) return true;
  const long long p = 2ll * max_radius;
  if (D + p > INT32_MAX || H + p > INT32_MAX || W + p > INT32_MAX) return false;
  return edt_dims_ok(1, (int)(D + p), (int)(H + p), (int)(W + p));
}

static PostWs post_ws(void* ws, int D, int H, int W, int max_radius) {
  PostWs r;
  r.clean = clean_ws(ws, (size_t)D * H * W);
  char* p = static_cast<char*>(ws);
  size_t off = r.clean.bytes;
  const size_t Sp = max_radius ? (size_t)(D + 2 * max_radius) * (H + 2 * max_radius) * (W + 2 * max_radius) : 0;
  r.ncomp = reinterpret_cast<long long*>(p + off); off += align16(2 * sizeof(long long));
  r.site = reinterpret_cast<uint8_t*>(p + off);    off += align16(Sp);
  r.sq = reinterpret_cast<int*>(p + off);          off += align16(Sp * sizeof(int));
  r.bytes = off;
  return r;
}

__device__ __forceinline__ bool clean_has(const CleanSet& set, uint32_t v) {
  return (set.w[v >> 6] >> (v & 63u)) & 1ull;
}

// two counts of a workgroup, each added by one 64-bit atomic (none for a zero)
__device__ __forceinline__ void post_add2(uint32_t a, uint32_t b, long long* dst) {
  __shared__ uint32_t red[CC_WAVES][2];
  a = cc_wave_sum(a);
  b = cc_wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = a;
    red[threadIdx.x >> 6][1] = b;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    uint32_t s = 0;
    for (int w = 0; w < CC_WAVES; ++w) s += red[w][threadIdx.x];
    if (s) atomicAdd(reinterpret_cast<unsigned long long*>(dst) + threadIdx.x, (unsigned long long)s);
  }
}

// fill: k_clean_mask with the test inverted - the complement plane, and the root marks zeroed.  VEC 4: map 4-B aligned
template <int VEC>
__global__ __launch_bounds__(CC_THREADS) void k_post_comp_mask(const uint8_t* __restrict__ map, CleanSet set, int S,
                                                               uint8_t* __restrict__ mask, int* __restrict__ marks) {
  const long long tid = (long long)blockIdx.x * CC_THREADS + threadIdx.x, step = (long long)gridDim.x * CC_THREADS;
  const long long groups = S / VEC;
  for (long long g = tid; g < groups; g += step) {
    if constexpr (VEC == 4) {
      const uchar4 v = *reinterpret_cast<const uchar4*>(map + 4 * g);
      *reinterpret_cast<uchar4*>(mask + 4 * g) =
          make_uchar4(!clean_has(set, v.x), !clean_has(set, v.y), !clean_has(set, v.z), !clean_has(set, v.w));
      *reinterpret_cast<int4*>(marks + 4 * g) = make_int4(0, 0, 0, 0);
    } else {
      mask[g] = (uint8_t)!clean_has(set, map[g]);
      marks[g] = 0;
    }
  }
  const long long i = groups * VEC + tid;          // the last S % VEC voxels one by one
  if (i < S) {
    mask[i] = (uint8_t)!clean_has(set, map[i]);
    marks[i] = 0;
  }
}

// fill: the voxels on the six faces, 2 (H W + D W + D H) of them (an edge voxel comes twice: the store is the same).
// labels: flattened, of the complement plane
__global__ __launch_bounds__(CC_THREADS) void k_post_faces(const int* __restrict__ labels, int D, int H, int W,
                                                           int* __restrict__ marks) {
  const long long HW = (long long)H * W, DW = (long long)D * W, DH = (long long)D * H;
  const long long total = 2 * (HW + DW + DH);
  for (long long f = (long long)blockIdx.x * CC_THREADS + threadIdx.x; f < total; f += (long long)gridDim.x * CC_THREADS) {
    long long v;
    if (f < 2 * HW) {
      v = (f < HW ? 0 : (D - 1) * HW) + f % HW;
    } else if (f < 2 * (HW + DW)) {
      const long long g = f - 2 * HW, rem = g % DW;
      v = ((rem / W) * H + (g < DW ? 0 : H - 1)) * W + rem % W;
    } else {
      const long long g = f - 2 * (HW + DW);
      v = (g % DH) * W + (g < DH ? 0 : W - 1);
    }
    const int l = labels[v];
    if (l) marks[l - 1] = 1;
  }
}

// fill: stats (2) = holes (roots without a mark), voxels relabelled
__global__ __launch_bounds__(CC_THREADS) void k_post_fill_apply(const int* __restrict__ labels,
                                                                const int* __restrict__ marks, int to, int S,
                                                                uint8_t* __restrict__ map, long long* __restrict__ stats) {
  uint32_t holes = 0, cnt = 0;
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const int l = labels[i];
    if (l == 0 || marks[l - 1] != 0) continue;
    map[i] = (uint8_t)to;
    ++cnt;
    if (l == (int)i + 1) ++holes;
  }
  post_add2(holes, cnt, stats);
}

// close / open: the sites of the volume's voxels inside the padded plane (the pad is a memset): M for close, its
// complement for open.  VEC 4: W % 4 == 0 and map 4-B aligned, so a group of four lies in one row
template <bool OPEN, int VEC>
__global__ __launch_bounds__(CC_THREADS) void k_post_sites(const uint8_t* __restrict__ map, CleanSet set, int S, int H,
                                                           int W, int rad, uint8_t* __restrict__ site) {
  const int Hp = H + 2 * rad, Wp = W + 2 * rad;
  const long long groups = S / VEC;                  // VEC 1 or S % 4 == 0
  for (long long g = (long long)blockIdx.x * CC_THREADS + threadIdx.x; g < groups; g += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)(g * VEC);
    const int w = v % W, q = v / W, h = q % H, d = q / H;
    uint8_t* dst = site + ((size_t)(d + rad) * Hp + h + rad) * Wp + w + rad;
    if constexpr (VEC == 4) {
      const uchar4 m = *reinterpret_cast<const uchar4*>(map + v);
      dst[0] = (uint8_t)(clean_has(set, m.x) != OPEN);
      dst[1] = (uint8_t)(clean_has(set, m.y) != OPEN);
      dst[2] = (uint8_t)(clean_has(set, m.z) != OPEN);
      dst[3] = (uint8_t)(clean_has(set, m.w) != OPEN);
    } else {
      dst[0] = (uint8_t)(clean_has(set, map[v]) != OPEN);
    }
  }
}

// close / open: the sites of the second transform, sq > R^2, over the whole padded plane (16-B loads, 4-B stores)
__global__ __launch_bounds__(CC_THREADS) void k_post_thresh(const int* __restrict__ sq, int Sp, int r2,
                                                            uint8_t* __restrict__ site) {
  const long long tid = (long long)blockIdx.x * CC_THREADS + threadIdx.x, step = (long long)gridDim.x * CC_THREADS;
  const long long groups = Sp / 4;
  for (long long g = tid; g < groups; g += step) {
    const int4 v = *reinterpret_cast<const int4*>(sq + 4 * g);
    *reinterpret_cast<uchar4*>(site + 4 * g) = make_uchar4(v.x > r2, v.y > r2, v.z > r2, v.w > r2);
  }
  const long long i = groups * 4 + tid;
  if (i < Sp) site[i] = (uint8_t)(sq[i] > r2);
}

// close: the voxels outside M with sq > R^2 become TO; open: the voxels of M with sq > R^2.  stats (2) = voxels of M
// before the rule, voxels relabelled.  VEC as k_post_sites
template <bool OPEN, int VEC>
__global__ __launch_bounds__(CC_THREADS) void k_post_ball_apply(const int* __restrict__ sq, CleanSet set, int S, int H,
                                                                int W, int rad, int r2, int to,
                                                                uint8_t* __restrict__ map, long long* __restrict__ stats) {
  const int Hp = H + 2 * rad, Wp = W + 2 * rad;
  const long long groups = S / VEC;
  uint32_t inside = 0, cnt = 0;
  for (long long g = (long long)blockIdx.x * CC_THREADS + threadIdx.x; g < groups; g += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)(g * VEC);
    const int w = v % W, q = v / W, h = q % H, d = q / H;
    const int* e = sq + ((size_t)(d + rad) * Hp + h + rad) * Wp + w + rad;
    uint8_t m[VEC];
    if constexpr (VEC == 4) {
      const uchar4 u = *reinterpret_cast<const uchar4*>(map + v);
      m[0] = u.x; m[1] = u.y; m[2] = u.z; m[3] = u.w;
    } else {
      m[0] = map[v];
    }
    uint32_t hit = 0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const bool in = clean_has(set, m[k]);
      inside += in;
      if (in == OPEN && e[k] > r2) {
        m[k] = (uint8_t)to;
        ++hit;
      }
    }
    if (hit) {
      if constexpr (VEC == 4) *reinterpret_cast<uchar4*>(map + v) = make_uchar4(m[0], m[1], m[2], m[3]);
      else map[v] = m[0];
      cnt += hit;
    }
  }
  post_add2(inside, cnt, stats);
}

static inline bool post_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// fill on the map `out`: 8 launches.  dual: the connectivity of the holes
static int post_fill_run(const PostWs& s, const CleanSet& set, int to, int D, int H, int W, int dual, uint8_t* out,
                         long long* stats, hipStream_t st) {
  const int S = D * H * W;
  const CleanWs& c = s.clean;
  const dim3 b(CC_THREADS), gs(cc_grid((size_t)S, CC_STREAM_BLOCKS));
  int* marks = c.sizes;
  if (post_aligned4(out))
    hipLaunchKernelGGL(k_post_comp_mask<4>, dim3(cc_grid((size_t)S / 4 + 1, CC_STREAM_BLOCKS)), b, 0, st, out, set, S,
                       c.mask, marks);
  else
    hipLaunchKernelGGL(k_post_comp_mask<1>, gs, b, 0, st, out, set, S, c.mask, marks);
  EFFQ_LAUNCH_CHECK();
  CcSrc src;
  src.masks = c.mask; src.bits = nullptr; src.C = 0;
  const int rc = cc_run(src, 1, D, H, W, dual, c.labels, nullptr, 0, c.partial, s.ncomp, st);
  if (rc != EFFQ_OK) return rc;
  const size_t faces = 2 * ((size_t)H * W + (size_t)D * W + (size_t)D * H);
  hipLaunchKernelGGL(k_post_faces, dim3(cc_grid(faces, CC_STREAM_BLOCKS)), b, 0, st, c.labels, D, H, W, marks);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_post_fill_apply, gs, b, 0, st, c.labels, marks, to, S, out, stats);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// close (OPEN false) or open of radius rad on the map `out`: a memset and 9 launches
template <bool OPEN>
static int post_ball_run(const PostWs& s, const CleanSet& set, int rad, int to, int D, int H, int W, uint8_t* out,
                         long long* stats, hipStream_t st) {
  const int S = D * H * W, r2 = rad * rad;
  const int Dp = D + 2 * rad, Hp = H + 2 * rad, Wp = W + 2 * rad, Sp = Dp * Hp * Wp;
  const dim3 b(CC_THREADS);
  const bool v4 = W % 4 == 0 && post_aligned4(out);
  const dim3 gs(cc_grid(v4 ? (size_t)S / 4 : (size_t)S, CC_STREAM_BLOCKS));
  EdtSrc src;
  src.masks = s.site; src.surf = nullptr; src.C = 0;
  EFFQ_HIP(hipMemsetAsync(s.site, OPEN ? 1 : 0, (size_t)Sp, st));
  if (v4) hipLaunchKernelGGL((k_post_sites<OPEN, 4>), gs, b, 0, st, out, set, S, H, W, rad, s.site);
  else hipLaunchKernelGGL((k_post_sites<OPEN, 1>), gs, b, 0, st, out, set, S, H, W, rad, s.site);
  EFFQ_LAUNCH_CHECK();
  int rc = edt_run<EdtVox>(src, 1, Dp, Hp, Wp, EdtUnit{}, EdtUnit{}, EdtUnit{}, s.sq, st);
  if (rc != EFFQ_OK) return rc;
  hipLaunchKernelGGL(k_post_thresh, dim3(cc_grid((size_t)Sp / 4 + 1, CC_STREAM_BLOCKS)), b, 0, st, s.sq, Sp, r2, s.site);
  EFFQ_LAUNCH_CHECK();
  rc = edt_run<EdtVox>(src, 1, Dp, Hp, Wp, EdtUnit{}, EdtUnit{}, EdtUnit{}, s.sq, st);
  if (rc != EFFQ_OK) return rc;
  if (v4) hipLaunchKernelGGL((k_post_ball_apply<OPEN, 4>), gs, b, 0, st, s.sq, set, S, H, W, rad, r2, to, out, stats);
  else hipLaunchKernelGGL((k_post_ball_apply<OPEN, 1>), gs, b, 0, st, s.sq, set, S, H, W, rad, r2, to, out, stats);
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
  if (ws_bytes < s.bytes) {
    set_error("effq_cc_label: workspace of %zu bytes, needs %zu", ws_bytes, s.bytes);
    return EFFQ_ERR_WORKSPACE;
  }
  CcSrc src;
  src.masks = masks; src.bits = nullptr; src.C = 0;
  return cc_run(src, P, D, H, W, connectivity, labels, nullptr, 0, s.partial, ncomp, as_stream(stream));
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
  if (ws_bytes < s.bytes) {
    set_error("effq_seg_lesions: workspace of %zu bytes, needs %zu", ws_bytes, s.bytes);
    return EFFQ_ERR_WORKSPACE;
  }
  const hipStream_t st = as_stream(stream);
  const int rc = cc_decision_bits(logits, label, C, S, mode, fuse, thresh, s.bits, st);
  if (rc != EFFQ_OK) return rc;
  CcSrc src;
  src.masks = nullptr; src.bits = s.bits; src.C = C;
  return cc_run(src, P, D, H, W, connectivity, s.labels, s.flags, C, s.partial, counts, st);
}

size_t effq_cc_table_ws_bytes(int P, int D, int H, int W, int max_rows) {
  if (!cc_dims_ok(P, D, H, W) || max_rows <= 0) return 0;
  return cc_table_ws(nullptr, P, (size_t)D * H * W).bytes;
}

int effq_cc_table(const uint8_t* masks, int P, int D, int H, int W, int connectivity, int max_rows, int32_t* rows,
                  long long* nrows, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(masks && rows && nrows && ws && max_rows > 0);
  EFFQ_CHECK_ARG(cc_dims_ok(P, D, H, W));
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  const CcTableWs t = cc_table_ws(ws, P, (size_t)D * H * W);
  if (ws_bytes < t.bytes) {
    set_error("effq_cc_table: workspace of %zu bytes, needs %zu", ws_bytes, t.bytes);
    return EFFQ_ERR_WORKSPACE;
  }
  const hipStream_t st = as_stream(stream);
  CcSrc src;
  src.masks = masks; src.bits = nullptr; src.C = 0;
  const int rc = cc_run(src, P, D, H, W, connectivity, t.cc.labels, nullptr, 0, t.cc.partial, nrows, st);
  if (rc != EFFQ_OK) return rc;
  return cc_table_run(t, nullptr, 0, P, D * H * W, max_rows, 2, rows, nrows, st);
}

int effq_seg_lesion_table(const float* logits, const uint8_t* label, int C, int D, int H, int W, int mode, int fuse,
                          float thresh, int connectivity, int max_rows, long long* counts, long long* nrows,
                          int32_t* rows, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(logits && label && counts && nrows && rows && ws && max_rows > 0);
  EFFQ_CHECK_ARG(C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(cc_dims_ok(2 * C, D, H, W));
  EFFQ_CHECK_ARG(mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID);
  EFFQ_CHECK_ARG(fuse == EFFQ_SEG_FUSE_NONE || fuse == EFFQ_SEG_FUSE_AGG || fuse == EFFQ_SEG_FUSE_CON);
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  const int P = 2 * C;
  const size_t S = (size_t)D * H * W;
  const CcTableWs t = cc_table_ws(ws, P, S);
  if (ws_bytes < t.bytes) {
    set_error("effq_seg_lesion_table: workspace of %zu bytes, needs %zu", ws_bytes, t.bytes);
    return EFFQ_ERR_WORKSPACE;
  }
  const hipStream_t st = as_stream(stream);
  int rc = cc_decision_bits(logits, label, C, S, mode, fuse, thresh, t.cc.bits, st);
  if (rc != EFFQ_OK) return rc;
  CcSrc src;
  src.masks = nullptr; src.bits = t.cc.bits; src.C = C;
  rc = cc_run(src, P, D, H, W, connectivity, t.cc.labels, t.cc.flags, C, t.cc.partial, counts, st);
  if (rc != EFFQ_OK) return rc;
  return cc_table_run(t, t.cc.bits, C, P, (int)S, max_rows, 3, rows, nrows, st);
}

size_t effq_label_clean_ws_bytes(int D, int H, int W) {
  if (!cc_dims_ok(1, D, H, W)) return 0;
  return clean_ws(nullptr, (size_t)D * H * W).bytes;
}

int effq_label_clean(const uint8_t* in, int D, int H, int W, int connectivity, int R, const uint8_t* sets,
                     const long long* rules, uint8_t* out, long long* stats, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(in && sets && rules && out && stats && ws);
  EFFQ_CHECK_ARG(R >= 1 && R <= EFFQ_LABEL_CLEAN_MAX_RULES);
  EFFQ_CHECK_ARG(cc_dims_ok(1, D, H, W));
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  CleanSet set[EFFQ_LABEL_CLEAN_MAX_RULES];
  for (int r = 0; r < R; ++r) {
    const long long op = rules[3 * r], n = rules[3 * r + 1], to = rules[3 * r + 2];
    EFFQ_CHECK_ARG(op == EFFQ_LABEL_CLEAN_LARGEST || op == EFFQ_LABEL_CLEAN_MIN);
    EFFQ_CHECK_ARG(op != EFFQ_LABEL_CLEAN_MIN || n >= 1);
    EFFQ_CHECK_ARG(to >= 0 && to <= 255);
    EFFQ_CHECK_ARG(sets[256 * r] == 0 && sets[256 * r + to] == 0);
    for (int k = 0; k < 4; ++k) set[r].w[k] = 0ull;
    for (int v = 0; v < 256; ++v)
      if (sets[256 * r + v]) set[r].w[v >> 6] |= 1ull << (v & 63);
  }
  const int S = D * H * W;
  const CleanWs s = clean_ws(ws, (size_t)S);
  if (ws_bytes < s.bytes) {
    set_error("effq_label_clean: workspace of %zu bytes, needs %zu", ws_bytes, s.bytes);
    return EFFQ_ERR_WORKSPACE;
  }
  const hipStream_t st = as_stream(stream);
  if (out != in) EFFQ_HIP(hipMemcpyAsync(out, in, (size_t)S, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_clean_init, dim3(1), dim3(64), 0, st, s.best, stats, R);
  EFFQ_LAUNCH_CHECK();
  for (int r = 0; r < R; ++r) {
    const int rc = clean_rule_run(s, set[r], rules + 3 * r, D, H, W, connectivity, out, stats + 2 * r, s.best + r, st);
    if (rc != EFFQ_OK) return rc;
  }
  return EFFQ_OK;
}

size_t effq_label_post_ws_bytes(int D, int H, int W, int max_radius) {
  if (!post_dims_ok(D, H, W, max_radius)) return 0;
  return post_ws(nullptr, D, H, W, max_radius).bytes;
}

int effq_label_post(const uint8_t* in, int D, int H, int W, int connectivity, int R, const uint8_t* sets,
                    const long long* rules, uint8_t* out, long long* stats, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(in && sets && rules && out && stats && ws);
  EFFQ_CHECK_ARG(R >= 1 && R <= EFFQ_LABEL_CLEAN_MAX_RULES);
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  CleanSet set[EFFQ_LABEL_CLEAN_MAX_RULES];
  int max_radius = 0;
  for (int r = 0; r < R; ++r) {
    const long long op = rules[3 * r], n = rules[3 * r + 1], to = rules[3 * r + 2];
    EFFQ_CHECK_ARG(op >= EFFQ_LABEL_CLEAN_LARGEST && op <= EFFQ_LABEL_POST_OPEN);
    EFFQ_CHECK_ARG(op != EFFQ_LABEL_CLEAN_MIN || n >= 1);
    const bool ball = op == EFFQ_LABEL_POST_CLOSE || op == EFFQ_LABEL_POST_OPEN;
    EFFQ_CHECK_ARG(!ball || (n >= 1 && n <= EFFQ_LABEL_POST_MAX_RADIUS));
    EFFQ_CHECK_ARG(to >= 0 && to <= 255);
    // fill and close add voxels to the mask: TO is one of its values; the other ops take voxels out of it
    const bool grows = op == EFFQ_LABEL_POST_FILL || op == EFFQ_LABEL_POST_CLOSE;
    EFFQ_CHECK_ARG(sets[256 * r] == 0 && (sets[256 * r + to] != 0) == grows);
    if (ball && n > max_radius) max_radius = (int)n;
    for (int k = 0; k < 4; ++k) set[r].w[k] = 0ull;
    for (int v = 0; v < 256; ++v)
      if (sets[256 * r + v]) set[r].w[v >> 6] |= 1ull << (v & 63);
  }
  EFFQ_CHECK_ARG(post_dims_ok(D, H, W, max_radius));
  const int S = D * H * W;
  const PostWs s = post_ws(ws, D, H, W, max_radius);
  if (ws_bytes < s.bytes) {
    set_error("effq_label_post: workspace of %zu bytes, needs %zu", ws_bytes, s.bytes);
    return EFFQ_ERR_WORKSPACE;
  }
  const hipStream_t st = as_stream(stream);
  if (out != in) EFFQ_HIP(hipMemcpyAsync(out, in, (size_t)S, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_clean_init, dim3(1), dim3(64), 0, st, s.clean.best, stats, R);
  EFFQ_LAUNCH_CHECK();
  for (int r = 0; r < R; ++r) {
    const long long op = rules[3 * r];
    const int n = (int)rules[3 * r + 1], to = (int)rules[3 * r + 2];
    int rc;
    if (op == EFFQ_LABEL_POST_FILL)
      rc = post_fill_run(s, set[r], to, D, H, W, connectivity == 26 ? 6 : 26, out, stats + 2 * r, st);
    else if (op == EFFQ_LABEL_POST_CLOSE)
      rc = post_ball_run<false>(s, set[r], n, to, D, H, W, out, stats + 2 * r, st);
    else if (op == EFFQ_LABEL_POST_OPEN)
      rc = post_ball_run<true>(s, set[r], n, to, D, H, W, out, stats + 2 * r, st);
    else
      rc = clean_rule_run(s.clean, set[r], rules + 3 * r, D, H, W, connectivity, out, stats + 2 * r, s.clean.best + r, st);
    if (rc != EFFQ_OK) return rc;
  }
  return EFFQ_OK;
}

}  // extern "C"
