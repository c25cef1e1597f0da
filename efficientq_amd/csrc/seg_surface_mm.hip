// The distance transform with per-axis weights and the surface distances in millimetres (effq_edt_sq_mm,
// effq_seg_surface_mm).  The contract - E(v, s) defined in fp32 term by term, the outputs - is in include/effq_hip.h; why
// the separable passes return the bits of the brute force, how the two pooled ranks are selected and what was measured is
// in DESIGN section 13 ("Source geometry").  Phases of a call, in launch order:
//   masks, surface   the decision bits (seg_masks.h) and the 6-neighbour stencil (seg_surf.h), as effq_seg_surface
//   rows, lines      the three separable passes of seg_surf.h with the metric EdtMm: fl(g(j) + fl(wa (i - j)^2)) in fp32
//   reduce           k_mm_scan, then k_mm_select / k_mm_hist over 8 + 8 + 8 + 8 bits of the pattern, k_mm_next, k_mm_final
// effq_label_surface_mm takes its decision bits from two label maps (label_bits.h) and runs the same launches after them
// (mm_surface_run); with tolerances it then counts the surface voxels within each: k_surf_within, k_surf_within_final
// (DESIGN section 26).
#include <cmath>

#include "common.h"
#include "label_bits.h"
#include "seg_decide.h"
#include "seg_masks.h"
#include "seg_surf.h"

namespace effq {

constexpr int MM_THREADS = 256;
constexpr int MM_ROWS = MM_THREADS / 64;               // waves of a workgroup of the scan
constexpr int MM_SCAN_BLOCKS = 1024;                   // blocks of the scans = per-block partials of the fp64 sums
constexpr int MM_BINS = 256;                           // 8 bits of the pattern per stage of the select
constexpr int MM_STAGES = 4;
constexpr int MM_CLASSES = EFFQ_SEG_TALLIES_MAX_CLASSES;
constexpr int MM_STATE = 8;                            // uint32 per class: the fields below
constexpr int ST_PREFIX = 0, ST_RANK = 1, ST_POOLED = 2, ST_NEXT = 3, ST_SAME = 4;
constexpr uint32_t MM_INF_BITS = 0x7f800000u;
static_assert(MM_CLASSES == 8, "rows of the reduce arrays");
static_assert((EFFQ_EDT_MM_MAX_EXTENT + 2) * sizeof(float) <= (size_t)EDT_LDS_AIM, "one line and its range fit the slab");

static inline size_t mm_align16(size_t n) { return (n + 15) & ~(size_t)15; }

// the small arrays of the reduce, sized for MM_CLASSES whatever C is
struct MmRed {
  uint32_t* hist;                // (MM_STAGES, MM_CLASSES, MM_BINS) pooled over both directions
  unsigned long long* cnt;       // (2 MM_CLASSES): row 2 c = nP, row 2 c + 1 = nL
  uint32_t* mx;                  // (2 MM_CLASSES) patterns of the largest finite E
  uint32_t* state;               // (MM_CLASSES, MM_STATE)
  double* part;                  // (MM_SCAN_BLOCKS, 2 MM_CLASSES)
};

struct MmWs {
  float* sq;                     // (P, S)
  uint16_t* bits;                // (S)
  uint16_t* surf;                // (S)
  char* zeroed;                  // hist, cnt, mx, state: cleared by one memset
  size_t zeroed_bytes;
  MmRed red;
  size_t bytes;
};

static MmWs mm_ws(void* ws, int P, int D, int H, int W) {
  MmWs r;
  const size_t S = (size_t)D * H * W;
  char* p = static_cast<char*>(ws);
  size_t off = 0;
  r.sq = reinterpret_cast<float*>(p + off);      off += mm_align16((size_t)P * S * sizeof(float));
  r.bits = reinterpret_cast<uint16_t*>(p + off); off += mm_align16(S * sizeof(uint16_t));
  r.surf = reinterpret_cast<uint16_t*>(p + off); off += mm_align16(S * sizeof(uint16_t));
  r.zeroed = p + off;
  r.red.hist = reinterpret_cast<uint32_t*>(p + off); off += (size_t)MM_STAGES * MM_CLASSES * MM_BINS * sizeof(uint32_t);
  r.red.cnt = reinterpret_cast<unsigned long long*>(p + off); off += 2 * MM_CLASSES * sizeof(unsigned long long);
  r.red.mx = reinterpret_cast<uint32_t*>(p + off);    off += 2 * MM_CLASSES * sizeof(uint32_t);
  r.red.state = reinterpret_cast<uint32_t*>(p + off); off += (size_t)MM_CLASSES * MM_STATE * sizeof(uint32_t);
  r.zeroed_bytes = (size_t)(p + off - r.zeroed);
  off = mm_align16(off);
  r.red.part = reinterpret_cast<double*>(p + off); off += (size_t)MM_SCAN_BLOCKS * 2 * MM_CLASSES * sizeof(double);
  r.bytes = off;
  return r;
}

// ---- reduce ---------------------------------------------------------------------------------------------------------
// The pattern of E at surface voxel i of row 2 c + dir: dir 0 = E_L over S(P) of class c, dir 1 = E_P over S(L).
__device__ __forceinline__ uint32_t mm_value(const float* __restrict__ sq, int C, size_t S, int c, int dir, size_t i) {
  return __float_as_uint(sq[(size_t)(dir ? c : C + c) * S + i]);
}

template <int C>
__global__ __launch_bounds__(MM_THREADS) void k_mm_scan(const uint16_t* __restrict__ surf, const float* __restrict__ sq,
                                                        int S, MmRed r) {
  constexpr int R = 2 * C;
  __shared__ uint32_t s_hist[C * MM_BINS];
  __shared__ double s_sum[MM_ROWS][R];
  __shared__ uint32_t s_cnt[MM_ROWS][R], s_max[MM_ROWS][R];
  for (int k = threadIdx.x; k < C * MM_BINS; k += MM_THREADS) s_hist[k] = 0;
  __syncthreads();
  double sum[R];
  uint32_t cnt[R], mx[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    sum[k] = 0.0;
    cnt[k] = mx[k] = 0;
  }
  for (long long i = (long long)blockIdx.x * MM_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * MM_THREADS) {
    const uint32_t b = surf[i];
    if (!b) continue;
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int dir = 0; dir < 2; ++dir) {
        if (!((b >> (dir ? 8 + c : c)) & 1)) continue;
        const uint32_t e = mm_value(sq, C, (size_t)S, c, dir, (size_t)i);
        ++cnt[2 * c + dir];
        atomicAdd(&s_hist[c * MM_BINS + (e >> 24)], 1u);
        if (e != MM_INF_BITS) {                        // +inf: the target has no surface
          mx[2 * c + dir] = max(mx[2 * c + dir], e);
          sum[2 * c + dir] += sqrt((double)__uint_as_float(e));
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < R; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sum[k] += __shfl_down(sum[k], off);
      cnt[k] += __shfl_down(cnt[k], off);
      mx[k] = max(mx[k], __shfl_down(mx[k], off));
    }
    if (lane == 0) {
      s_sum[wave][k] = sum[k];
      s_cnt[wave][k] = cnt[k];
      s_max[wave][k] = mx[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < R) {
    const int k = threadIdx.x;
    double s = 0.0;
    unsigned long long n = 0;
    uint32_t m = 0;
    for (int v = 0; v < MM_ROWS; ++v) {
      s += s_sum[v][k];
      n += s_cnt[v][k];
      m = max(m, s_max[v][k]);
    }
    r.part[(size_t)blockIdx.x * 2 * MM_CLASSES + k] = s;
    if (n) atomicAdd(&r.cnt[k], n);
    if (m) atomicMax(&r.mx[k], m);
  }
  for (int k = threadIdx.x; k < C * MM_BINS; k += MM_THREADS)
    if (s_hist[k]) atomicAdd(&r.hist[k], s_hist[k]);   // stage 0: (c, bin) = k
}

// One workgroup per class, one thread per bin of stage `stage`: the bin that holds the rank still sought extends the
// prefix by 8 bits.  Stage 0 first places the rank from the counts.
__global__ __launch_bounds__(MM_BINS) void k_mm_select(MmRed r, int stage) {
  __shared__ uint32_t s_scan[MM_BINS];
  __shared__ uint32_t s_rank, s_go;
  const int c = blockIdx.x, t = threadIdx.x;
  uint32_t* st = r.state + c * MM_STATE;
  if (t == 0) {
    if (stage == 0) {
      const unsigned long long n_p = r.cnt[2 * c], n_l = r.cnt[2 * c + 1];
      const bool pooled = n_p > 0 && n_l > 0;
      st[ST_PREFIX] = 0;
      st[ST_RANK] = pooled ? (uint32_t)(95ull * (n_p + n_l - 1) / 100ull) : 0u;
      st[ST_POOLED] = pooled;
      st[ST_NEXT] = 0xFFFFFFFFu;
      st[ST_SAME] = 0;
    }
    s_rank = st[ST_RANK];
    s_go = st[ST_POOLED];
  }
  __syncthreads();
  if (!s_go) return;
  const uint32_t k = r.hist[((size_t)stage * MM_CLASSES + c) * MM_BINS + t];
  s_scan[t] = k;
  __syncthreads();
  for (int off = 1; off < MM_BINS; off <<= 1) {
    const uint32_t v = t >= off ? s_scan[t - off] : 0u;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  const uint32_t incl = s_scan[t], excl = incl - k, rank = s_rank;
  if (excl <= rank && rank < incl) {                   // one thread
    st[ST_PREFIX] |= (uint32_t)t << (24 - 8 * stage);
    st[ST_RANK] = rank - excl;
    if (stage == MM_STAGES - 1) st[ST_SAME] = rank - excl + 1 < k;       // rank lo + 1 holds the same value
  }
}

// stage 1..3: the values whose leading 8 * stage bits equal the prefix, counted by their next 8 bits
__global__ __launch_bounds__(MM_THREADS) void k_mm_hist(const uint16_t* __restrict__ surf, const float* __restrict__ sq,
                                                        int C, int S, MmRed r, int stage) {
  __shared__ uint32_t s_hist[MM_CLASSES * MM_BINS];
  __shared__ uint32_t s_pref[MM_CLASSES], s_on[MM_CLASSES];
  if (threadIdx.x < MM_CLASSES) {
    const bool on = threadIdx.x < C && r.state[threadIdx.x * MM_STATE + ST_POOLED];
    s_on[threadIdx.x] = on;
    s_pref[threadIdx.x] = on ? r.state[threadIdx.x * MM_STATE + ST_PREFIX] : 0u;
  }
  for (int k = threadIdx.x; k < C * MM_BINS; k += MM_THREADS) s_hist[k] = 0;
  __syncthreads();
  const int shift = 32 - 8 * stage;
  for (long long i = (long long)blockIdx.x * MM_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * MM_THREADS) {
    const uint32_t b = surf[i];
    if (!b) continue;
    for (int c = 0; c < C; ++c) {
      if (!s_on[c]) continue;
#pragma unroll
      for (int dir = 0; dir < 2; ++dir) {
        if (!((b >> (dir ? 8 + c : c)) & 1)) continue;
        const uint32_t e = mm_value(sq, C, (size_t)S, c, dir, (size_t)i);
        if ((e >> shift) == (s_pref[c] >> shift)) atomicAdd(&s_hist[c * MM_BINS + ((e >> (shift - 8)) & 255u)], 1u);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < C * MM_BINS; k += MM_THREADS)
    if (s_hist[k]) atomicAdd(&r.hist[(size_t)stage * MM_CLASSES * MM_BINS + k], s_hist[k]);
}

// the smallest pattern above the value of rank lo, for the classes whose rank lo + 1 is not that value again
__global__ __launch_bounds__(MM_THREADS) void k_mm_next(const uint16_t* __restrict__ surf, const float* __restrict__ sq,
                                                        int C, int S, MmRed r) {
  __shared__ uint32_t s_min[MM_CLASSES], s_lo[MM_CLASSES], s_on[MM_CLASSES], s_any;
  if (threadIdx.x == 0) s_any = 0;
  __syncthreads();
  if (threadIdx.x < MM_CLASSES) {
    const uint32_t* st = r.state + threadIdx.x * MM_STATE;
    const bool on = threadIdx.x < C && st[ST_POOLED] && !st[ST_SAME];
    s_on[threadIdx.x] = on;
    s_lo[threadIdx.x] = on ? st[ST_PREFIX] : 0u;
    s_min[threadIdx.x] = 0xFFFFFFFFu;
    if (on) s_any = 1;
  }
  __syncthreads();
  if (!s_any) return;
  for (long long i = (long long)blockIdx.x * MM_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * MM_THREADS) {
    const uint32_t b = surf[i];
    if (!b) continue;
    for (int c = 0; c < C; ++c) {
      if (!s_on[c]) continue;
#pragma unroll
      for (int dir = 0; dir < 2; ++dir) {
        if (!((b >> (dir ? 8 + c : c)) & 1)) continue;
        const uint32_t e = mm_value(sq, C, (size_t)S, c, dir, (size_t)i);
        if (e > s_lo[c] && e < s_min[c]) atomicMin(&s_min[c], e);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < C && s_min[threadIdx.x] != 0xFFFFFFFFu)
    atomicMin(&r.state[threadIdx.x * MM_STATE + ST_NEXT], s_min[threadIdx.x]);
}

// One workgroup per class: the per-block partials of both sums added in block order (thread t takes blocks t, t + 256,
// ..., then a fixed tree), and the outputs written.
__global__ __launch_bounds__(MM_THREADS) void k_mm_final(MmRed r, int nblocks, long long* __restrict__ counts,
                                                         float* __restrict__ sq_out, double* __restrict__ sums) {
  __shared__ double s_red[MM_THREADS];
  const int c = blockIdx.x, t = threadIdx.x;
  for (int dir = 0; dir < 2; ++dir) {
    const int row = 2 * c + dir;
    double s = 0.0;
    for (int b = t; b < nblocks; b += MM_THREADS) s += r.part[(size_t)b * 2 * MM_CLASSES + row];
    s_red[t] = s;
    __syncthreads();
    for (int off = MM_THREADS / 2; off > 0; off >>= 1) {
      if (t < off) s_red[t] += s_red[t + off];
      __syncthreads();
    }
    if (t == 0) {
      sums[row] = s_red[0];
      counts[row] = (long long)r.cnt[row];
      sq_out[4 * c + dir] = __uint_as_float(r.mx[row]);
    }
    __syncthreads();
  }
  if (t == 0) {
    const uint32_t* st = r.state + c * MM_STATE;
    const bool pooled = st[ST_POOLED];
    sq_out[4 * c + 2] = pooled ? __uint_as_float(st[ST_PREFIX]) : 0.0f;
    sq_out[4 * c + 3] = pooled ? __uint_as_float(st[ST_SAME] ? st[ST_PREFIX] : st[ST_NEXT]) : 0.0f;
  }
}

// ---- surface voxels within a tolerance (effq_label_surface_mm) --------------------------------------------------------
constexpr int MM_TOLS = EFFQ_SURF_TOL_MAX;
constexpr int MM_WITHIN = 2 * MM_CLASSES * (MM_TOLS + 1);              // counters: (row 2 c + dir, first tolerance)
static_assert(MM_WITHIN == 144, "the LDS counters of k_surf_within");

struct MmTols {
  float sq[MM_TOLS];             // ascending; entries n .. are unused
  int n;
};

// A surface voxel of row 2 c + dir adds 1 at the first tolerance that holds its stored distance (fp32 <=), at n when
// none does (+inf among them): the tolerances ascend, so that is the number of tolerances it exceeds.  LDS counters per
// workgroup, then integer adds into the workspace.  One voxel per lane, as k_mm_scan walks the surface bits: the
// distances of neighbouring surface voxels of a row are then read by neighbouring lanes.
__global__ __launch_bounds__(MM_THREADS) void k_surf_within(const uint16_t* __restrict__ surf,
                                                            const float* __restrict__ sq, int C, int S, MmTols tol,
                                                            unsigned long long* __restrict__ within) {
  __shared__ uint32_t s_cnt[MM_WITHIN];
  for (int k = threadIdx.x; k < MM_WITHIN; k += MM_THREADS) s_cnt[k] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * MM_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * MM_THREADS) {
    const uint32_t b = surf[i];
    if (!b) continue;
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int dir = 0; dir < 2; ++dir) {
        if (!((b >> (dir ? 8 + c : c)) & 1)) continue;
        const float e = __uint_as_float(mm_value(sq, C, (size_t)S, c, dir, (size_t)i));
        int first = 0;
#pragma unroll
        for (int k = 0; k < MM_TOLS; ++k) first += (k < tol.n && !(e <= tol.sq[k])) ? 1 : 0;
        atomicAdd(&s_cnt[(2 * c + dir) * (MM_TOLS + 1) + first], 1u);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < MM_WITHIN; k += MM_THREADS)
    if (s_cnt[k]) atomicAdd(&within[k], (unsigned long long)s_cnt[k]);
}

// out (C, 2, n): the prefix sums over the tolerances of the counters of row 2 c + dir, one thread per row
__global__ __launch_bounds__(64) void k_surf_within_final(const unsigned long long* __restrict__ within, int C, int n,
                                                          long long* __restrict__ out) {
  const int row = threadIdx.x;
  if (row >= 2 * C) return;
  unsigned long long run = 0;
  for (int k = 0; k < n; ++k) {
    run += within[row * (MM_TOLS + 1) + k];
    out[(size_t)row * n + k] = (long long)run;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
static bool mm_dims_ok(int P, int D, int H, int W) {
  return P > 0 && P <= 65535 && D > 0 && H > 0 && W > 0 && D <= EFFQ_EDT_MM_MAX_EXTENT && H <= EFFQ_EDT_MM_MAX_EXTENT &&
         W <= EFFQ_EDT_MM_MAX_EXTENT && (long long)P * D * H * W < (1ll << 31);
}

static bool mm_weight_ok(float w) { return std::isfinite(w) && w > 0.0f; }

template <int C>
static void launch_scan(dim3 g, hipStream_t st, const uint16_t* surf, const float* sq, int S, const MmRed& r) {
  hipLaunchKernelGGL((k_mm_scan<C>), g, dim3(MM_THREADS), 0, st, surf, sq, S, r);
}

// Everything after the decision bits in s.bits (the counters of s already cleared): surface stencil, the three passes,
// scan, select / hist, next, final.  One sequence for the bits of logits and of label maps.
static int mm_surface_run(const MmWs& s, int C, int D, int H, int W, float wd, float wh, float ww, long long* counts,
                          float* sq, double* sums, hipStream_t st) {
  const int P = 2 * C;
  const size_t S = (size_t)D * H * W;
  const dim3 gs(cc_grid(S, CC_STREAM_BLOCKS)), b(CC_THREADS);
  hipLaunchKernelGGL(k_surf_bits, gs, b, 0, st, s.bits, s.surf, D, H, W);
  EFFQ_LAUNCH_CHECK();
  EdtSrc src;
  src.masks = nullptr; src.surf = s.surf; src.C = C;
  const int rc = edt_run<EdtMm>(src, P, D, H, W, wd, wh, ww, s.sq, st);
  if (rc != EFFQ_OK) return rc;
  const dim3 g(cc_grid(S, MM_SCAN_BLOCKS)), t(MM_THREADS);
  switch (C) {
    case 1: launch_scan<1>(g, st, s.surf, s.sq, (int)S, s.red); break;
    case 2: launch_scan<2>(g, st, s.surf, s.sq, (int)S, s.red); break;
    case 3: launch_scan<3>(g, st, s.surf, s.sq, (int)S, s.red); break;
    case 4: launch_scan<4>(g, st, s.surf, s.sq, (int)S, s.red); break;
    case 5: launch_scan<5>(g, st, s.surf, s.sq, (int)S, s.red); break;
    case 6: launch_scan<6>(g, st, s.surf, s.sq, (int)S, s.red); break;
    case 7: launch_scan<7>(g, st, s.surf, s.sq, (int)S, s.red); break;
    default: launch_scan<8>(g, st, s.surf, s.sq, (int)S, s.red); break;
  }
  EFFQ_LAUNCH_CHECK();
  for (int stage = 0; stage < MM_STAGES; ++stage) {
    if (stage > 0) {
      hipLaunchKernelGGL(k_mm_hist, g, t, 0, st, s.surf, s.sq, C, (int)S, s.red, stage);
      EFFQ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_mm_select, dim3(C), dim3(MM_BINS), 0, st, s.red, stage);
    EFFQ_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_mm_next, g, t, 0, st, s.surf, s.sq, C, (int)S, s.red);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mm_final, dim3(C), t, 0, st, s.red, (int)g.x, counts, sq, sums);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// the workspace of effq_label_surface_mm: that of effq_seg_surface_mm, then the counters of k_surf_within
static size_t mm_within_offset(int C, int D, int H, int W) { return mm_align16(mm_ws(nullptr, 2 * C, D, H, W).bytes); }
constexpr size_t MM_WITHIN_BYTES = MM_WITHIN * sizeof(unsigned long long);

static bool mm_tols_ok(const float* tol_sq, int ntol) {
  if (ntol < 0 || ntol > MM_TOLS || (ntol > 0 && !tol_sq)) return false;
  for (int k = 0; k < ntol; ++k)
    if (!std::isfinite(tol_sq[k]) || tol_sq[k] < 0.0f || (k > 0 && !(tol_sq[k] > tol_sq[k - 1]))) return false;
  return true;
}

}  // namespace effq
using namespace effq;

extern "C" {

size_t effq_surf_mm_ws_bytes(int P, int D, int H, int W) {
  if (!mm_dims_ok(P, D, H, W)) return 0;
  return mm_ws(nullptr, P, D, H, W).bytes;
}

int effq_edt_sq_mm(const uint8_t* masks, int P, int D, int H, int W, float wd, float wh, float ww, float* sq, void* ws,
                   size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(masks && sq && ws);
  EFFQ_CHECK_ARG(mm_dims_ok(P, D, H, W));
  EFFQ_CHECK_ARG(mm_weight_ok(wd) && mm_weight_ok(wh) && mm_weight_ok(ww));
  EFFQ_CHECK_ARG(ws_bytes >= mm_ws(ws, P, D, H, W).bytes);
  EdtSrc src;
  src.masks = masks; src.surf = nullptr; src.C = 0;
  return edt_run<EdtMm>(src, P, D, H, W, wd, wh, ww, sq, as_stream(stream));
}

int effq_seg_surface_mm(const float* logits, const uint8_t* label, int C, int D, int H, int W, int mode, int fuse,
                        float thresh, float wd, float wh, float ww, long long* counts, float* sq, double* sums, void* ws,
                        size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(logits && label && counts && sq && sums && ws && C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(mm_dims_ok(2 * C, D, H, W));
  EFFQ_CHECK_ARG(mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID);
  EFFQ_CHECK_ARG(fuse == EFFQ_SEG_FUSE_NONE || fuse == EFFQ_SEG_FUSE_AGG || fuse == EFFQ_SEG_FUSE_CON);
  EFFQ_CHECK_ARG(mm_weight_ok(wd) && mm_weight_ok(wh) && mm_weight_ok(ww));
  const int P = 2 * C;
  const size_t S = (size_t)D * H * W;
  const MmWs s = mm_ws(ws, P, D, H, W);
  EFFQ_CHECK_ARG(ws_bytes >= s.bytes);
  const hipStream_t st = as_stream(stream);
  EFFQ_HIP(hipMemsetAsync(s.zeroed, 0, s.zeroed_bytes, st));
  const int rc = cc_decision_bits(logits, label, C, S, mode, fuse, thresh, s.bits, st);
  if (rc != EFFQ_OK) return rc;
  return mm_surface_run(s, C, D, H, W, wd, wh, ww, counts, sq, sums, st);
}

size_t effq_label_surface_mm_ws_bytes(int C, int D, int H, int W, int ntol) {
  if (C <= 0 || C > EFFQ_SEG_TALLIES_MAX_CLASSES || ntol < 0 || ntol > MM_TOLS || !mm_dims_ok(2 * C, D, H, W)) return 0;
  return mm_within_offset(C, D, H, W) + MM_WITHIN_BYTES;
}

int effq_label_surface_mm(const uint8_t* pred, const uint8_t* truth, int C, int D, int H, int W, const uint16_t* lut,
                          float wd, float wh, float ww, const float* tol_sq, int ntol, long long* counts, float* sq,
                          double* sums, long long* within, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(pred && truth && lut && counts && sq && sums && ws && C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(mm_dims_ok(2 * C, D, H, W));
  EFFQ_CHECK_ARG(mm_weight_ok(wd) && mm_weight_ok(wh) && mm_weight_ok(ww));
  EFFQ_CHECK_ARG(mm_tols_ok(tol_sq, ntol) && (ntol == 0 || within));
  EFFQ_CHECK_ARG(label_lut_ok(lut, C));
  EFFQ_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0);          // 8-B loads of the surface bits, 8-B counters
  EFFQ_CHECK_ARG(ws_bytes >= effq_label_surface_mm_ws_bytes(C, D, H, W, ntol));
  const size_t S = (size_t)D * H * W;
  const MmWs s = mm_ws(ws, 2 * C, D, H, W);
  const hipStream_t st = as_stream(stream);
  EFFQ_HIP(hipMemsetAsync(s.zeroed, 0, s.zeroed_bytes, st));
  int rc = label_decision_bits(pred, truth, lut, S, s.bits, st);
  if (rc != EFFQ_OK) return rc;
  rc = mm_surface_run(s, C, D, H, W, wd, wh, ww, counts, sq, sums, st);
  if (rc != EFFQ_OK || ntol == 0) return rc;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(static_cast<char*>(ws) + mm_within_offset(C, D, H, W));
  EFFQ_HIP(hipMemsetAsync(cnt, 0, MM_WITHIN_BYTES, st));
  MmTols tol;
  tol.n = ntol;
  for (int k = 0; k < MM_TOLS; ++k) tol.sq[k] = k < ntol ? tol_sq[k] : 0.0f;
  // the grid of the scans: every workgroup ends with up to 2 C (ntol + 1) adds on the same few words
  hipLaunchKernelGGL(k_surf_within, dim3(cc_grid(S, MM_SCAN_BLOCKS)), dim3(MM_THREADS), 0, st, s.surf, s.sq, C, (int)S,
                     tol, cnt);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_surf_within_final, dim3(1), dim3(64), 0, st, cnt, C, ntol, within);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
