// One geometric record per lesion of one or two uint8 label maps (effq_label_lesion_measures: `score --lesion_measures`,
// `predict --lesion_measures`): the sums of the coordinates, the box and the two farthest pairs of voxels of every
// connected component.  The contract is in include/effq_hip.h, the argument in DESIGN section 28.  Launches of a call:
//
//   bits            k_label_bits (label_bits.h); without a truth map the predicted map stands in for it
//   label .. final  cc_run of seg_cc.hip on those bits
//   chunks .. accum cc_table_run of seg_cc_table.hip: rows (first voxel, size, overlap), label words -> rows
//   init            the records of the rows that exist and the per-row words of the workspace
//   moments         every voxel of a row adds its coordinates to the row's sums and widens its box (LDS slots per
//                   workgroup, then int64 atomics on the record), and counts the row's candidates: the voxels that end a
//                   line of the component along w (along h when the slices are stacked along w)
//   scan            one workgroup: exclusive scans of the candidates and of the tile pairs of all rows
//   scatter         the candidates of every row, compacted row by row (in no fixed order inside a row)
//   pairs           workgroups stride over the tile pairs (i <= j) of all rows: tile j in LDS, one candidate of tile i
//                   per thread; the greatest E and, among equals, the least smaller index a, as one 64-bit atomicMax on
//                   E's bits << 32 | (2^31 - 1 - a), for the 3-D pair and for the pairs inside one slice
//   partner         every candidate whose E to a equals the greatest E offers itself as b: atomicMin
// A call whose rows have more than EFFQ_LESION_MEASURE_MAX_TILE_PAIRS tile pairs in all does not search them (the work
// grows with the square of the line ends of a component): its end points are -1, everything else is complete.
//
// Integer atomics only; the winner of every atomic is decided by values, not by arrival: equal inputs give equal bits.
// The order of the compacted candidates varies from run to run and never reaches an output.
#include "common.h"
#include "label_bits.h"
#include "seg_cc.h"

#include <math.h>

namespace effq {

constexpr int MEAS_WORDS = EFFQ_LESION_MEASURE_WORDS;
constexpr int MEAS_TILE = CC_THREADS;                  // candidates per tile: one per thread
constexpr int MEAS_PAIR_BLOCKS = 2048;                 // pairs: workgroups at most, they stride over the tile pairs
constexpr int MEAS_SLOTS = 256;                        // moments: rows a workgroup keeps in LDS (direct-mapped)
constexpr unsigned long long MEAS_MAX_TILE_PAIRS = EFFQ_LESION_MEASURE_MAX_TILE_PAIRS;   // of all rows of a call
constexpr long long MEAS_NONE = 0x7fffffffll;          // above every coordinate and every voxel index
static_assert(MEAS_WORDS == 13, "sums 0..2, box 3..8, pair 9..10, in-plane pair 11..12");

struct MeasWs {
  CcTableWs t;
  unsigned long long* pair_off;   // (N + 1) exclusive scan of the tile pairs; N = P * max_rows
  unsigned long long* best;       // (N, 2) E bits << 32 | MEAS_NONE - a: the 3-D pair, the in-plane pair
  uint32_t* ncand;                // (N)
  uint32_t* cursor;               // (N)
  uint32_t* cand_off;             // (N + 1) exclusive scan of ncand
  int* cand;                      // (P * S) the candidates (voxel indices), row after row
  size_t bytes;
};

static MeasWs meas_ws(void* ws, int P, size_t S, int max_rows) {
  MeasWs r;
  r.t = cc_table_ws(ws, P, S);
  const size_t N = (size_t)P * max_rows;
  char* p = static_cast<char*>(ws);
  size_t off = r.t.bytes;
  r.pair_off = reinterpret_cast<unsigned long long*>(p + off); off += align16((N + 1) * sizeof(unsigned long long));
  r.best = reinterpret_cast<unsigned long long*>(p + off);     off += align16(N * 2 * sizeof(unsigned long long));
  r.ncand = reinterpret_cast<uint32_t*>(p + off);              off += align16(N * sizeof(uint32_t));
  r.cursor = reinterpret_cast<uint32_t*>(p + off);             off += align16(N * sizeof(uint32_t));
  r.cand_off = reinterpret_cast<uint32_t*>(p + off);           off += align16((N + 1) * sizeof(uint32_t));
  r.cand = reinterpret_cast<int*>(p + off);                    off += align16((size_t)P * S * sizeof(int));
  r.bytes = off;
  return r;
}

static bool meas_dims_ok(int C, int planes, int D, int H, int W, int max_rows) {
  if (C <= 0 || C > EFFQ_SEG_TALLIES_MAX_CLASSES || (planes != C && planes != 2 * C)) return false;
  if (!cc_dims_ok(planes, D, H, W) || max_rows <= 0 || (long long)planes * max_rows >= (1ll << 31)) return false;
  return D <= EFFQ_EDT_MM_MAX_EXTENT && H <= EFFQ_EDT_MM_MAX_EXTENT && W <= EFFQ_EDT_MM_MAX_EXTENT;
}

struct MeasGrid {
  int D, H, W, S, max_rows;
  int line_h;                     // the lines run along h (slices stacked along w), else along w
  float wd, wh, ww;
};

// E of the offsets between two voxels, term by term in fp32 (the Makefile builds with -ffp-contract=off)
__device__ __forceinline__ float meas_energy(const MeasGrid& g, int dd, int dh, int dw) {
  return (g.wd * (float)(dd * dd) + g.wh * (float)(dh * dh)) + g.ww * (float)(dw * dw);
}

__device__ __forceinline__ void meas_coords(const MeasGrid& g, int v, int& d, int& h, int& w) {
  w = v % g.W;
  const int q = v / g.W;
  h = q % g.H;
  d = q / g.H;
}

// a foreground voxel that ends a line of its component: adjacent foreground voxels of a plane share a component at
// either connectivity, so the neighbours along the line decide
__device__ __forceinline__ bool meas_line_end(const MeasGrid& g, const int* __restrict__ L, int v, int h, int w) {
  const int c = g.line_h ? h : w, n = g.line_h ? g.H : g.W, step = g.line_h ? g.W : 1;
  return c == 0 || c == n - 1 || L[v - step] == 0 || L[v + step] == 0;
}

__device__ __forceinline__ unsigned long long meas_key(float e, int a) {
  return ((unsigned long long)__float_as_uint(e) << 32) | (unsigned long long)(MEAS_NONE - a);
}

// ---- init -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void k_meas_init(const long long* __restrict__ nrows, int max_rows, int N,
                                                          long long* __restrict__ meas, uint32_t* __restrict__ ncand,
                                                          uint32_t* __restrict__ cursor,
                                                          unsigned long long* __restrict__ best) {
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * CC_THREADS) {
    const int e = (int)i;
    ncand[e] = 0;
    cursor[e] = 0;
    best[2 * (size_t)e] = 0;
    best[2 * (size_t)e + 1] = 0;
    if (e % max_rows >= nrows[e / max_rows]) continue;
    long long* m = meas + (size_t)e * MEAS_WORDS;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      m[a] = 0;
      m[3 + a] = MEAS_NONE;
      m[6 + a] = 0;
    }
    m[9] = 0;
    m[10] = MEAS_NONE;
    m[11] = 0;
    m[12] = MEAS_NONE;
  }
}

// ---- moments --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void meas_record_add(long long* __restrict__ m, uint32_t* __restrict__ nc,
                                                const unsigned long long (&sum)[3], const int (&lo)[3],
                                                const int (&hi)[3], uint32_t n) {
  unsigned long long* u = reinterpret_cast<unsigned long long*>(m);      // every word of a record is >= 0
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicAdd(u + a, sum[a]);
    atomicMin(u + 3 + a, (unsigned long long)lo[a]);
    atomicMax(u + 6 + a, (unsigned long long)hi[a]);
  }
  if (n) atomicAdd(nc, n);
}

__global__ __launch_bounds__(CC_THREADS) void k_meas_moments(const int* __restrict__ labels, MeasGrid g,
                                                             long long* __restrict__ meas,
                                                             uint32_t* __restrict__ ncand) {
  __shared__ int s_key[MEAS_SLOTS];
  __shared__ unsigned long long s_sum[3][MEAS_SLOTS];
  __shared__ int s_lo[3][MEAS_SLOTS], s_hi[3][MEAS_SLOTS];
  __shared__ uint32_t s_nc[MEAS_SLOTS];
  const int plane = blockIdx.y;
  const int* L = labels + (size_t)plane * g.S;
  long long* M = meas + (size_t)plane * g.max_rows * MEAS_WORDS;
  uint32_t* NC = ncand + (size_t)plane * g.max_rows;
  for (int k = threadIdx.x; k < MEAS_SLOTS; k += CC_THREADS) {
    s_key[k] = -1;
    s_nc[k] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s_sum[a][k] = 0;
      s_lo[a][k] = (int)MEAS_NONE;
      s_hi[a][k] = 0;
    }
  }
  __syncthreads();
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < g.S; i += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)i;
    const int l = L[v];
    if (l == 0) continue;
    const int r = cc_row(L, l);
    if (r >= g.max_rows) continue;
    int c[3];
    meas_coords(g, v, c[0], c[1], c[2]);
    const uint32_t end = meas_line_end(g, L, v, c[1], c[2]) ? 1u : 0u;
    const int s = r & (MEAS_SLOTS - 1);
    int k = s_key[s];
    if (k == -1) {
      k = atomicCAS(&s_key[s], -1, r);
      if (k == -1) k = r;
    }
    if (k == r) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicAdd(&s_sum[a][s], (unsigned long long)c[a]);
        atomicMin(&s_lo[a][s], c[a]);
        atomicMax(&s_hi[a][s], c[a]);
      }
      if (end) atomicAdd(&s_nc[s], 1u);
    } else {                               // the slot belongs to another row
      const unsigned long long sum[3] = {(unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2]};
      meas_record_add(M + (size_t)r * MEAS_WORDS, NC + r, sum, c, c, end);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < MEAS_SLOTS; k += CC_THREADS) {
    const int r = s_key[k];
    if (r < 0) continue;
    const unsigned long long sum[3] = {s_sum[0][k], s_sum[1][k], s_sum[2][k]};
    const int lo[3] = {s_lo[0][k], s_lo[1][k], s_lo[2][k]}, hi[3] = {s_hi[0][k], s_hi[1][k], s_hi[2][k]};
    meas_record_add(M + (size_t)r * MEAS_WORDS, NC + r, sum, lo, hi, s_nc[k]);
  }
}

// ---- scan -----------------------------------------------------------------------------------------------------------
// one workgroup: thread t owns a run of consecutive rows; the runs are scanned in LDS.  A row of n candidates has
// T = ceil(n / MEAS_TILE) tiles and T (T + 1) / 2 tile pairs.
__global__ __launch_bounds__(CC_THREADS) void k_meas_scan(const uint32_t* __restrict__ ncand, int N,
                                                          uint32_t* __restrict__ cand_off,
                                                          unsigned long long* __restrict__ pair_off) {
  __shared__ uint32_t s_c[CC_THREADS];
  __shared__ unsigned long long s_p[CC_THREADS];
  const int t = threadIdx.x;
  const int per = (N + CC_THREADS - 1) / CC_THREADS;
  const int b0 = (int)min((long long)N, (long long)t * per), b1 = (int)min((long long)N, (long long)b0 + per);
  auto pairs_of = [](uint32_t n) {
    const unsigned long long T = (n + MEAS_TILE - 1) / MEAS_TILE;
    return T * (T + 1) / 2;
  };
  uint32_t c = 0;
  unsigned long long p = 0;
  for (int b = b0; b < b1; ++b) {
    c += ncand[b];
    p += pairs_of(ncand[b]);
  }
  s_c[t] = c;
  s_p[t] = p;
  __syncthreads();
  for (int o = 1; o < CC_THREADS; o <<= 1) {
    const uint32_t ac = t >= o ? s_c[t - o] : 0u;
    const unsigned long long ap = t >= o ? s_p[t - o] : 0ull;
    __syncthreads();
    s_c[t] += ac;
    s_p[t] += ap;
    __syncthreads();
  }
  uint32_t rc = s_c[t] - c;               // exclusive
  unsigned long long rp = s_p[t] - p;
  for (int b = b0; b < b1; ++b) {
    const uint32_t n = ncand[b];
    cand_off[b] = rc;
    pair_off[b] = rp;
    rc += n;
    rp += pairs_of(n);
  }
  if (t == CC_THREADS - 1) {
    cand_off[N] = s_c[t];
    pair_off[N] = s_p[t];
  }
}

// ---- scatter --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void k_meas_scatter(const int* __restrict__ labels, MeasGrid g,
                                                             const uint32_t* __restrict__ cand_off,
                                                             uint32_t* __restrict__ cursor, int* __restrict__ cand) {
  const int plane = blockIdx.y;
  const int* L = labels + (size_t)plane * g.S;
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < g.S; i += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)i;
    const int l = L[v];
    if (l == 0) continue;
    const int r = cc_row(L, l);
    if (r >= g.max_rows) continue;
    int d, h, w;
    meas_coords(g, v, d, h, w);
    if (!meas_line_end(g, L, v, h, w)) continue;
    const size_t e = (size_t)plane * g.max_rows + r;
    cand[cand_off[e] + atomicAdd(&cursor[e], 1u)] = v;
  }
}

// the last index e of off (N + 1 ascending words) with off[e] <= x, for x < off[N]: the row that holds item x
template <typename T>
__device__ __forceinline__ int meas_row_of(const T* __restrict__ off, int N, T x) {
  int lo = 0, hi = N;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (off[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- pairs ----------------------------------------------------------------------------------------------------------
// AX: the axis the slices are stacked along.  A thread keeps its bests while its workgroup stays in one row and hands them
// over when the row changes: wave maximum, then one atomicMax per wave and kind.
__device__ __forceinline__ void meas_flush(unsigned long long* __restrict__ best, int e, float b3, int a3, float b2,
                                           int a2) {
  long long k3 = b3 < 0.f ? 0ll : (long long)meas_key(b3, a3);         // E >= 0: the sign bit is clear
  long long k2 = b2 < 0.f ? 0ll : (long long)meas_key(b2, a2);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    k3 = max(k3, __shfl_xor(k3, o, 64));
    k2 = max(k2, __shfl_xor(k2, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    if (k3) atomicMax(&best[2 * (size_t)e], (unsigned long long)k3);
    if (k2) atomicMax(&best[2 * (size_t)e + 1], (unsigned long long)k2);
  }
}

template <int AX>
__global__ __launch_bounds__(CC_THREADS) void k_meas_pairs(const int* __restrict__ cand,
                                                           const uint32_t* __restrict__ cand_off,
                                                           const unsigned long long* __restrict__ pair_off, int N,
                                                           MeasGrid g, unsigned long long* __restrict__ best) {
  __shared__ int4 s_t[MEAS_TILE];                      // tile j: d, h, w, voxel
  const unsigned long long total = pair_off[N];
  if (total > MEAS_MAX_TILE_PAIRS) return;             // every workgroup alike: the partner pass marks the records
  const int t = threadIdx.x;
  int e = -1;
  unsigned long long lo = 0, hi = 0;                   // the tile pairs of row e
  uint32_t base = 0, n = 0;                            // its candidates
  float b3 = -1.f, b2 = -1.f;
  int a3 = 0, a2 = 0;
  for (unsigned long long wi = blockIdx.x; wi < total; wi += gridDim.x) {
    if (wi < lo || wi >= hi) {                         // the same for every thread of the workgroup
      if (e >= 0) meas_flush(best, e, b3, a3, b2, a2);
      b3 = b2 = -1.f;
      e = meas_row_of(pair_off, N, wi);
      lo = pair_off[e];
      hi = pair_off[e + 1];
      base = cand_off[e];
      n = cand_off[e + 1] - base;
    }
    // tile pair (i, j), i <= j, of local index j (j + 1) / 2 + i
    const unsigned long long local = wi - lo;
    unsigned long long j = (unsigned long long)((sqrt(8.0 * (double)local + 1.0) - 1.0) * 0.5);
    while (j * (j + 1) / 2 > local) --j;
    while ((j + 1) * (j + 2) / 2 <= local) ++j;
    const unsigned long long i = local - j * (j + 1) / 2;
    const uint32_t i0 = (uint32_t)i * MEAS_TILE, j0 = (uint32_t)j * MEAS_TILE;
    const int ni = (int)min((uint32_t)MEAS_TILE, n - i0), nj = (int)min((uint32_t)MEAS_TILE, n - j0);
    __syncthreads();                                   // the readers of the tile before are done
    if (t < nj) {
      const int v = cand[base + j0 + t];
      int d, h, w;
      meas_coords(g, v, d, h, w);
      s_t[t] = make_int4(d, h, w, v);
    }
    int v = 0, d = 0, h = 0, w = 0;
    if (t < ni) {
      v = cand[base + i0 + t];
      meas_coords(g, v, d, h, w);
    }
    __syncthreads();
    if (t < ni) {
      const int s = AX == 0 ? d : AX == 1 ? h : w;
#pragma unroll 4
      for (int k = 0; k < nj; ++k) {
        const int4 o = s_t[k];
        const float E = meas_energy(g, d - o.x, h - o.y, w - o.z);
        const int os = AX == 0 ? o.x : AX == 1 ? o.y : o.z;
        if (E >= b3) {                                 // rare after the first few: the ties are settled by the index
          const int a = min(v, o.w);
          if (E > b3 || a < a3) {
            b3 = E;
            a3 = a;
          }
        }
        if (os == s && E >= b2) {
          const int a = min(v, o.w);
          if (E > b2 || a < a2) {
            b2 = E;
            a2 = a;
          }
        }
      }
    }
  }
  if (e >= 0) meas_flush(best, e, b3, a3, b2, a2);
}

// ---- partner --------------------------------------------------------------------------------------------------------
// a is the least index that any pair of the greatest E holds, so every voxel at that E from a lies at or above it
template <int AX>
__global__ __launch_bounds__(CC_THREADS) void k_meas_partner(const int* __restrict__ cand,
                                                             const uint32_t* __restrict__ cand_off,
                                                             const unsigned long long* __restrict__ pair_off, int N,
                                                             MeasGrid g, const unsigned long long* __restrict__ best,
                                                             long long* __restrict__ meas) {
  const uint32_t total = cand_off[N];
  const bool skipped = pair_off[N] > MEAS_MAX_TILE_PAIRS;     // the pairs were not searched: the end points are -1
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * CC_THREADS) {
    const int e = meas_row_of(cand_off, N, (uint32_t)i);
    const int v = cand[i];
    int d, h, w;
    meas_coords(g, v, d, h, w);
    long long* m = meas + (size_t)e * MEAS_WORDS;
    if (skipped) {                                     // every candidate of the row stores the same four words
      m[9] = m[10] = m[11] = m[12] = -1;
      continue;
    }
#pragma unroll
    for (int kind = 0; kind < 2; ++kind) {
      const unsigned long long key = best[2 * (size_t)e + kind];
      const int a = (int)(MEAS_NONE - (long long)(key & 0xffffffffull));
      int ad, ah, aw;
      meas_coords(g, a, ad, ah, aw);
      if (v == a) m[9 + 2 * kind] = a;
      if (kind == 1 && (AX == 0 ? d != ad : AX == 1 ? h != ah : w != aw)) continue;
      if (__float_as_uint(meas_energy(g, d - ad, h - ah, w - aw)) != (uint32_t)(key >> 32)) continue;
      atomicMin(reinterpret_cast<unsigned long long*>(m + 10 + 2 * kind), (unsigned long long)v);
    }
  }
}

template <int AX>
static int meas_pairs_run(const MeasWs& s, int N, const MeasGrid& g, long long* meas, hipStream_t st) {
  const dim3 b(CC_THREADS);
  hipLaunchKernelGGL(k_meas_pairs<AX>, dim3(MEAS_PAIR_BLOCKS), b, 0, st, s.cand, s.cand_off, s.pair_off, N, g, s.best);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_meas_partner<AX>, dim3(CC_STREAM_BLOCKS), b, 0, st, s.cand, s.cand_off, s.pair_off, N, g, s.best,
                     meas);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // namespace effq
using namespace effq;

extern "C" {

size_t effq_label_lesion_measures_ws_bytes(int C, int planes, int D, int H, int W, int max_rows) {
  if (!meas_dims_ok(C, planes, D, H, W, max_rows)) return 0;
  return meas_ws(nullptr, planes, (size_t)D * H * W, max_rows).bytes;
}

int effq_label_lesion_measures(const uint8_t* pred, const uint8_t* truth, int C, int D, int H, int W,
                               const uint16_t* lut, int connectivity, float wd, float wh, float ww, int slice_axis,
                               int max_rows, long long* counts, long long* nrows, int32_t* rows, long long* meas,
                               void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(pred && lut && nrows && rows && meas && ws && (counts || !truth));
  const int P = truth ? 2 * C : C;
  EFFQ_CHECK_ARG(meas_dims_ok(C, P, D, H, W, max_rows));
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  EFFQ_CHECK_ARG(slice_axis >= 0 && slice_axis <= 2);
  EFFQ_CHECK_ARG(isfinite(wd) && isfinite(wh) && isfinite(ww) && wd > 0.f && wh > 0.f && ww > 0.f);
  EFFQ_CHECK_ARG(label_lut_ok(lut, C));
  const size_t S = (size_t)D * H * W;
  const MeasWs s = meas_ws(ws, P, S, max_rows);
  EFFQ_CHECK_WS(ws_bytes, s.bytes);
  const hipStream_t st = as_stream(stream);
  const CcWs& cc = s.t.cc;
  int rc = label_decision_bits(pred, truth ? truth : pred, lut, S, cc.bits, st);
  if (rc != EFFQ_OK) return rc;
  // without a truth map: plain labelling of the C predicted planes (cc_run leaves their component counts in nrows, which
  // the table's scan writes again), no flags and no overlap
  if (truth) rc = cc_run(cc_src_bits(cc.bits, C), P, D, H, W, connectivity, cc.labels, cc.flags, C, cc.partial, counts, st);
  else rc = cc_run(cc_src_bits(cc.bits, C), P, D, H, W, connectivity, cc.labels, nullptr, 0, cc.partial, nrows, st);
  if (rc != EFFQ_OK) return rc;
  rc = cc_table_run(s.t, truth ? cc.bits : nullptr, C, P, (int)S, max_rows, 3, rows, nrows, st);
  if (rc != EFFQ_OK) return rc;

  const int N = P * max_rows;
  MeasGrid g;
  g.D = D; g.H = H; g.W = W; g.S = (int)S; g.max_rows = max_rows;
  g.line_h = slice_axis == 2;
  g.wd = wd; g.wh = wh; g.ww = ww;
  const dim3 b(CC_THREADS), gs(cc_grid(S, CC_STREAM_BLOCKS), P);
  hipLaunchKernelGGL(k_meas_init, dim3(cc_grid((size_t)N, CC_STREAM_BLOCKS)), b, 0, st, nrows, max_rows, N, meas, s.ncand,
                     s.cursor, s.best);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_meas_moments, gs, b, 0, st, cc.labels, g, meas, s.ncand);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_meas_scan, dim3(1), b, 0, st, s.ncand, N, s.cand_off, s.pair_off);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_meas_scatter, gs, b, 0, st, cc.labels, g, s.cand_off, s.cursor, s.cand);
  EFFQ_LAUNCH_CHECK();
  switch (slice_axis) {
    case 0: return meas_pairs_run<0>(s, N, g, meas, st);
    case 1: return meas_pairs_run<1>(s, N, g, meas, st);
    default: return meas_pairs_run<2>(s, N, g, meas, st);
  }
}

}  // extern "C"
