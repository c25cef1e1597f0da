// effq_prep_smooth: the separable Gaussian of `--prep_antialias` (prep.py), applied on the source grid before
// effq_prep_resample down-samples it.  x (N, D, H, W) fp32 -> y of the same shape; along every filtered axis
//   y[i] = sum_k g_|k| x[clamp(i + k, 0, n - 1)],  k = -r .. r,
// the edge replicated as lin_axis of prep.hip clamps it.  One launch per filtered axis, W then H then D, fp32 between
// the passes; each pass reads its input once from HBM (the 2 r + 1 shifted reads of a voxel are neighbours' reads and
// stay in the caches) and writes its output once.  Streaming, the idiom of prep.hip: a thread owns four consecutive w
// of one row and moves them as one 16-B vector of 4-B alignment; the last item of a row with W % 4 != 0 goes voxel by
// voxel.
//   H and D passes: a tap is the same four w of another row, so every tap is one coalesced vector load at a clamped row
//     index (two per k: the rows i - k and i + k share g_k).
//   W pass: the 4 + 2 r inputs of an item are read once into registers as 1 + 2 ceil(r / 4) aligned groups of four
//     (a group that leaves the row goes voxel by voxel at clamped indices) and the four outputs are formed from that
//     window; the window's size is a template parameter (r <= 4, 8, 16, 32) so that it stays in registers.
// Arithmetic of one output, in every pass: acc = g_0 x[i], then for k = 1 .. r: acc = fmaf(g_k, x[i - k] + x[i + k], acc).
// The taps come by value in the launch parameters (33 floats), read through scalar loads.  The grid depends on the
// extents alone, there is no reduction and no atomic: equal inputs give equal bits.  Every index is 32-bit (prep_fits).
#include "common.h"
#include "prep_rows.h"

namespace effq {

constexpr int SMOOTH_MAXR = EFFQ_PREP_SMOOTH_MAX_RADIUS;

struct SmoothParams {
  const float* x;
  float* y;
  const float* zero;        // the input of the whole call when this is the last pass of a keep_zero call, else null
  unsigned N, D, H, W;
  unsigned ext, stride;     // rows passes: the extent of the filtered axis and the distance of two of its rows
  int axis;                 // rows passes: 0 = D, 1 = H
  int r;
  float g[SMOOTH_MAXR + 1];      // centre first
};

// four consecutive voxels at `q`, the first `nv` of them inside the row (nv = 4: one 16-B load)
__device__ __forceinline__ void load_item(const float* __restrict__ q, unsigned nv, float (&v)[4]) {
  if (nv == 4) {
    const PFloat4 a = *reinterpret_cast<const PFloat4*>(q);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else {
#pragma unroll
    for (unsigned u = 0; u < 4; ++u) v[u] = u < nv ? q[u] : 0.0f;
  }
}

// out[u] where zero[u] == 0 becomes +0.0f (keep_zero), then the first nv values are stored at `dst`
__device__ __forceinline__ void store_item(float* __restrict__ dst, const float* __restrict__ zero, unsigned nv,
                                           float (&out)[4]) {
  if (zero) {
    float z[4];
    load_item(zero, nv, z);
#pragma unroll
    for (int u = 0; u < 4; ++u) out[u] = z[u] == 0.0f ? 0.0f : out[u];
  }
  if (nv == 4) {
    PFloat4 o;
    o.x = out[0]; o.y = out[1]; o.z = out[2]; o.w = out[3];
    *reinterpret_cast<PFloat4*>(dst) = o;
  } else {
#pragma unroll
    for (unsigned u = 0; u < 4; ++u)
      if (u < nv) dst[u] = out[u];
  }
}

// ---- along H or D: a tap is a whole-row shift --------------------------------------------------------------------------
__global__ __launch_bounds__(PREP_THREADS) void k_prep_smooth_rows(SmoothParams p) {
  const unsigned gw = (p.W + 3) / 4, total = p.N * p.D * p.H * gw;
  for (unsigned e = blockIdx.x * PREP_THREADS + threadIdx.x; e < total; e += gridDim.x * PREP_THREADS) {
    const RowItem it = row_item(e, gw, p.D, p.H);
    const unsigned pos = p.axis == 0 ? it.d : it.h;
    const unsigned base = ((it.n * p.D + it.d) * p.H + it.h) * p.W + it.w0;
    const unsigned nv = min(4u, p.W - it.w0);
    float c[4], acc[4];
    load_item(p.x + base, nv, c);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = p.g[0] * c[u];
    for (int k = 1; k <= p.r; ++k) {
      const unsigned lo = pos >= (unsigned)k ? pos - k : 0u, hi = min(pos + k, p.ext - 1);
      float a[4], b[4];
      load_item(p.x + (base - (pos - lo) * p.stride), nv, a);
      load_item(p.x + (base + (hi - pos) * p.stride), nv, b);
      const float gk = p.g[k];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = fmaf(gk, a[u] + b[u], acc[u]);
    }
    store_item(p.y + base, p.zero ? p.zero + base : nullptr, nv, acc);
  }
}

// ---- along W: the window of an item in registers --------------------------------------------------------------------------
template <int RB>
__global__ __launch_bounds__(PREP_THREADS) void k_prep_smooth_w(SmoothParams p) {
  constexpr int HG = RB / 4, NG = 1 + 2 * HG, NV = 4 * NG;      // groups -HG .. HG around the item's own
  const unsigned gw = (p.W + 3) / 4, total = p.N * p.D * p.H * gw;
  const int r = p.r, far = (r + 3) / 4, Wi = (int)p.W;          // the groups -far .. far hold the 4 + 2 r inputs
  for (unsigned e = blockIdx.x * PREP_THREADS + threadIdx.x; e < total; e += gridDim.x * PREP_THREADS) {
    const unsigned row = e / gw, w0 = (e - row * gw) * 4;
    const float* __restrict__ src = p.x + row * p.W;
    float v[NV];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const int jj = j - HG, ws = (int)w0 + 4 * jj;
      if (jj < -far || jj > far) {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[4 * j + u] = 0.0f;       // never read: every tap k <= r stays inside -far .. far
      } else if (ws >= 0 && ws + 4 <= Wi) {
        const PFloat4 a = *reinterpret_cast<const PFloat4*>(src + ws);
        v[4 * j] = a.x; v[4 * j + 1] = a.y; v[4 * j + 2] = a.z; v[4 * j + 3] = a.w;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[4 * j + u] = src[min(max(ws + u, 0), Wi - 1)];
      }
    }
    float out[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      constexpr int C0 = 4 * HG;                                // v[C0 + u] is output u's own voxel
      float acc = p.g[0] * v[C0 + u];
#pragma unroll
      for (int k = 1; k <= RB; ++k)
        if (k <= r) acc = fmaf(p.g[k], v[C0 + u - k] + v[C0 + u + k], acc);
      out[u] = acc;
    }
    const unsigned base = row * p.W + w0;
    store_item(p.y + base, p.zero ? p.zero + base : nullptr, min(4u, p.W - w0), out);
  }
}

static inline bool disjoint(const void* a, const void* b, uintptr_t bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa + bytes <= pb || pb + bytes <= pa;
}
static inline bool taps_ok(const float* g, int r) {
  if (r == 0) return true;
  if (!g) return false;
  for (int k = 0; k <= r; ++k)
    if (!(g[k] > 0.0f && g[k] <= 1.0f)) return false;          // false for a NaN
  return true;
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_prep_smooth(const float* x, int N, int D, int H, int W, const float* taps_d, int rd, const float* taps_h, int rh,
                     const float* taps_w, int rw, int keep_zero, float* y, float* tmp, void* stream) {
  EFFQ_CHECK_ARG(x && y && prep_fits(N, D, H, W) && (keep_zero == 0 || keep_zero == 1));
  EFFQ_CHECK_ARG(rd >= 0 && rd <= SMOOTH_MAXR && rh >= 0 && rh <= SMOOTH_MAXR && rw >= 0 && rw <= SMOOTH_MAXR);
  const int nf = (rd > 0) + (rh > 0) + (rw > 0);
  EFFQ_CHECK_ARG(nf > 0 && (nf == 1 || tmp));
  EFFQ_CHECK_ARG(taps_ok(taps_d, rd) && taps_ok(taps_h, rh) && taps_ok(taps_w, rw));
  const uintptr_t bytes = (uintptr_t)N * D * H * W * sizeof(float);
  EFFQ_CHECK_ARG(aligned_to(x, 4) && aligned_to(y, 4) && disjoint(x, y, bytes));
  EFFQ_CHECK_ARG(!tmp || (aligned_to(tmp, 4) && disjoint(x, tmp, bytes) && disjoint(y, tmp, bytes)));
  const hipStream_t st = as_stream(stream);
  const dim3 g(prep_grid((size_t)N * D * H * ((W + 3) / 4))), t(PREP_THREADS);
  SmoothParams p;
  p.N = N; p.D = D; p.H = H; p.W = W;
  const float* src = x;
  int pass = 0;
  // the last pass writes y, the one before it tmp, the first of three y
  auto begin = [&](const float* taps, int r) {
    float* dst = (nf - 1 - pass) % 2 == 0 ? y : tmp;
    p.x = src; p.y = dst; p.r = r;
    p.zero = keep_zero && pass == nf - 1 ? x : nullptr;
    for (int k = 0; k <= SMOOTH_MAXR; ++k) p.g[k] = k <= r ? taps[k] : 0.0f;
    src = dst;
    ++pass;
  };
  if (rw > 0) {
    begin(taps_w, rw);
    p.ext = W; p.stride = 1; p.axis = 2;
    if (rw <= 4) hipLaunchKernelGGL(k_prep_smooth_w<4>, g, t, 0, st, p);
    else if (rw <= 8) hipLaunchKernelGGL(k_prep_smooth_w<8>, g, t, 0, st, p);
    else if (rw <= 16) hipLaunchKernelGGL(k_prep_smooth_w<16>, g, t, 0, st, p);
    else hipLaunchKernelGGL(k_prep_smooth_w<32>, g, t, 0, st, p);
    EFFQ_LAUNCH_CHECK();
  }
  if (rh > 0) {
    begin(taps_h, rh);
    p.ext = H; p.stride = W; p.axis = 1;
    hipLaunchKernelGGL(k_prep_smooth_rows, g, t, 0, st, p);
    EFFQ_LAUNCH_CHECK();
  }
  if (rd > 0) {
    begin(taps_d, rd);
    p.ext = D; p.stride = (unsigned)H * W; p.axis = 0;
    hipLaunchKernelGGL(k_prep_smooth_rows, g, t, 0, st, p);
    EFFQ_LAUNCH_CHECK();
  }
  return EFFQ_OK;
}

}  // extern "C"
