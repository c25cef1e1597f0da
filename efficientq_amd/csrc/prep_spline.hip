// effq_prep_resample_cubic: the cubic B-spline resampling of `--prep_interp cubic` (prep.py; the rule is stated there and
// restated in include/effq_hip.h).  x (N, D, H, W) fp32 -> y (N, OD, OH, OW) fp32 through fp64 coefficients in `ws`
// (8 B per source voxel).  Four launches:
//   1 prefilter along D   k_prep_spline_lines<float>: reads x, writes ws (an axis of extent 1 is only converted);
//   2 prefilter along H   k_prep_spline_lines<double>: in place in ws;
//   3 prefilter along W   k_prep_spline_w: in place in ws, rows staged through LDS;
//   4 evaluation          k_prep_resample_cubic: 4 x 4 x 4 coefficients per output voxel, summed in fp64, one rounding.
// The prefilter of one line of extent n >= 2, pole z = sqrt(3) - 2, all in fp64 (nothing is fused: -ffp-contract=off):
//   s = sum of z^k xm[k] over one period k = 0 .. 2 n - 3 of the mirrored line xm (xm[k] = x[k] for k < n, x[2 n - 2 - k]
//     after it), added in that order, the powers formed by repeated multiplication; the walk stops where the power has
//     underflowed to exactly 0, since every later term is 0: no horizon is cut short;
//   c+[0] = 6 s / (1 - z^(2 n - 2));  c+[k] = 6 x[k] + z c+[k - 1];
//   c[n - 1] = z / (z^2 - 1) (c+[n - 1] + z c+[n - 2]);  c[k] = z (c[k + 1] - c+[k]).
// D and H passes: one thread per line, neighbouring threads on neighbouring w, so every load and store of the walks is
// coalesced; the line is walked for s (up to ~570 voxels from each end), forward for c+ and backward for c.
// W pass: the recursion runs along the contiguous axis.  A workgroup of 256 threads takes a tile of SPL_ROWS = 128 rows
// and walks it in chunks of SPL_CHUNK = 31 voxels: the chunk of every row is loaded with coalesced 8-B loads (a wave
// covers two rows' chunks per instruction) into tile[128][31] doubles (31 KB, five workgroups per CU), thread r < 128
// walks row r of the tile, and the chunk is stored back the same way.  The pitch of 31 doubles is odd, so the 32 lanes of
// a half wave, which walk 32 rows at one column, touch the dwords 62 r + 2 k: all 64 banks once.  The state of the
// recursion (the power and s, then c+[k - 1], then c[k + 1]) is carried in registers from chunk to chunk, forward for s
// and c+, backward for the mirrored half of s and for c: any W is the exact recursion, no halo.  (Tiles of 256 rows, a
// row per thread, were slower: 62 KB leave two workgroups per CU to hide the loads behind the walks, and a BraTS
// subject's 582 tiles then run as one full round of 512 and a nearly empty second one.)
// Evaluation: the shape of k_prep_resample_linear (four output voxels along W per thread, one 16-B store).
// No atomics, no reductions across threads, the grids depend on the extents alone: equal inputs give equal bits.
#include "common.h"
#include "prep_rows.h"

namespace effq {

constexpr int SPL_CHUNK = 31;                // voxels of a row per visit of the W pass
constexpr int SPL_ROWS = 128;                // rows of a tile: thread r < SPL_ROWS walks row r
constexpr int SPL_COLS = SPL_CHUNK + 1;      // staging: thread t moves column t % SPL_COLS (the last one idles) ...
constexpr int SPL_STAGE_ROWS = PREP_THREADS / SPL_COLS;      // ... of the rows t / SPL_COLS, + SPL_STAGE_ROWS, ...
static_assert(SPL_CHUNK % 2 == 1 && (SPL_COLS & (SPL_COLS - 1)) == 0 && PREP_THREADS % SPL_COLS == 0,
              "an odd pitch in doubles keeps the walks off one bank");
static_assert(SPL_ROWS <= PREP_THREADS && PREP_THREADS % SPL_ROWS == 0, "a thread per row of the tile");
static_assert(4 * SPL_ROWS * SPL_CHUNK * sizeof(double) <= 128 * 1024, "four workgroups per CU");

__device__ __forceinline__ double spline_pole() { return __builtin_sqrt(3.0) - 2.0; }

struct LineParams {
  const void* src;      // float (x) or double (ws itself)
  double* ws;
  unsigned lines, ext, stride;      // line e starts at (e / stride) ext stride + e % stride, its voxels `stride` apart
};

template <typename T>
__global__ __launch_bounds__(PREP_THREADS) void k_prep_spline_lines(LineParams p) {
  const double z = spline_pole(), last = z / (z * z - 1.0);
  const unsigned n = p.ext;
  const size_t st = p.stride;
  for (unsigned e = blockIdx.x * PREP_THREADS + threadIdx.x; e < p.lines; e += gridDim.x * PREP_THREADS) {
    const unsigned outer = e / p.stride, inner = e - outer * p.stride;
    const size_t base = (size_t)outer * n * st + inner;
    const T* x = static_cast<const T*>(p.src) + base;      // may be c itself: every voxel is read before it is written
    double* c = p.ws + base;
    if (n == 1) {
      c[0] = (double)x[0];
      continue;
    }
    double zk = 1.0, s = 0.0;
    for (unsigned k = 0; k < n && zk != 0.0; ++k) {
      s += zk * (double)x[k * st];
      zk *= z;
    }
    for (unsigned k = n - 2; k >= 1 && zk != 0.0; --k) {
      s += zk * (double)x[k * st];
      zk *= z;
    }
    double cp = (6.0 * s) / (1.0 - zk), prev = cp;           // zk = z^(2 n - 2), or 0 where that has underflowed
    for (unsigned k = 1; k < n; ++k) {
      const double v = (double)x[k * st];
      c[(k - 1) * st] = cp;
      prev = cp;
      cp = 6.0 * v + z * cp;
    }
    double cn = last * (cp + z * prev);
    c[(n - 1) * st] = cn;
    for (unsigned k = n - 1; k-- > 0;) {
      cn = z * (cn - c[k * st]);
      c[k * st] = cn;
    }
  }
}

__global__ __launch_bounds__(PREP_THREADS) void k_prep_spline_w(double* __restrict__ ws, unsigned rows, unsigned W) {
  __shared__ double tile[SPL_ROWS][SPL_CHUNK];
  const double z = spline_pole(), last = z / (z * z - 1.0);
  const unsigned nch = (W + SPL_CHUNK - 1) / SPL_CHUNK, ntiles = (rows + SPL_ROWS - 1) / SPL_ROWS;
  const unsigned t = threadIdx.x, col = t % SPL_COLS, r0 = t / SPL_COLS;
  for (unsigned tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const unsigned row0 = tl * SPL_ROWS, nr = min((unsigned)SPL_ROWS, rows - row0);
    const bool mine = t < nr;
    double* __restrict__ g = ws + (size_t)row0 * W;
    auto load = [&](unsigned j) {
      const unsigned w = j * SPL_CHUNK + col;
      if (col < SPL_CHUNK && w < W)
        for (unsigned r = r0; r < nr; r += SPL_STAGE_ROWS) tile[r][col] = g[(size_t)r * W + w];
    };
    auto store = [&](unsigned j) {
      const unsigned w = j * SPL_CHUNK + col;
      if (col < SPL_CHUNK && w < W)
        for (unsigned r = r0; r < nr; r += SPL_STAGE_ROWS) g[(size_t)r * W + w] = tile[r][col];
    };
    __syncthreads();                                          // the walks of the tile before are over
    // s: forward over the row, then backward over the voxels W - 2 .. 1.  zk is the same number in every thread, so
    // the whole workgroup leaves a loop together.
    double zk = 1.0, s = 0.0;
    for (unsigned j = 0; j < nch && zk != 0.0; ++j) {
      load(j);
      __syncthreads();
      const unsigned kn = min((unsigned)SPL_CHUNK, W - j * SPL_CHUNK);
      for (unsigned i = 0; i < kn; ++i) {
        if (mine) s += zk * tile[t][i];
        zk *= z;
      }
      __syncthreads();
    }
    for (unsigned j = nch; j-- > 0 && zk != 0.0;) {
      load(j);
      __syncthreads();
      const unsigned k0 = j * SPL_CHUNK, kn = min((unsigned)SPL_CHUNK, W - k0);
      for (unsigned i = kn; i-- > 0;) {
        const unsigned k = k0 + i;
        if (k >= 1 && k + 2 <= W) {
          if (mine) s += zk * tile[t][i];
          zk *= z;
        }
      }
      __syncthreads();
    }
    // c+, forward; a thread loads and stores the same voxels of the tile, so one barrier on each side of the walk
    double cp = (6.0 * s) / (1.0 - zk), prev = cp;
    for (unsigned j = 0; j < nch; ++j) {
      load(j);
      __syncthreads();
      if (mine) {
        const unsigned kn = min((unsigned)SPL_CHUNK, W - j * SPL_CHUNK);
        for (unsigned i = 0; i < kn; ++i) {
          if (j + i > 0) {
            prev = cp;
            cp = 6.0 * tile[t][i] + z * cp;
          }
          tile[t][i] = cp;
        }
      }
      __syncthreads();
      store(j);
    }
    // c, backward
    double cn = 0.0;
    for (unsigned j = nch; j-- > 0;) {
      load(j);
      __syncthreads();
      if (mine) {
        const unsigned k0 = j * SPL_CHUNK, kn = min((unsigned)SPL_CHUNK, W - k0);
        for (unsigned i = kn; i-- > 0;) {
          cn = k0 + i == W - 1 ? last * (cp + z * prev) : z * (cn - tile[t][i]);
          tile[t][i] = cn;
        }
      }
      __syncthreads();
      store(j);
    }
  }
}

// ---- evaluation --------------------------------------------------------------------------------------------------------
struct CubicParams {
  const float* x;
  const double* c;
  float* y;
  unsigned N, D, H, W, OD, OH, OW;
  double fd, fh, fw;
  int zero_keep;
};

// Output index o of an axis of source extent n: the coordinate of lin_axis (prep.hip); the four coefficient indices
// i0 - 1 .. i0 + 2, mirrored into the line, and their weights; i1 = the second index of the trilinear footprint.
__device__ __forceinline__ void cubic_axis(unsigned o, double f, unsigned n, unsigned (&idx)[4], double (&w)[4],
                                           unsigned& i0, unsigned& i1) {
  double s = ((double)o + 0.5) * f - 0.5;
  const double top = (double)(n - 1);
  s = s < 0.0 ? 0.0 : (s > top ? top : s);
  const double fl = floor(s), t = s - fl;
  const int b = (int)fl, ni = (int)n;
  i0 = (unsigned)b;
  i1 = i0 + (t > 0.0 && b < ni - 1 ? 1u : 0u);
  if (n == 1) {
    idx[0] = idx[1] = idx[2] = idx[3] = 0;
    w[0] = 0.0; w[1] = 1.0; w[2] = 0.0; w[3] = 0.0;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int i = b - 1 + j;
    i = i < 0 ? -i : i;
    i = i >= ni ? 2 * ni - 2 - i : i;
    idx[j] = (unsigned)min(max(i, 0), ni - 1);      // n = 2 and i0 + 2 = n + 1: outside twice, its weight is 0
  }
  const double t2 = t * t, t3 = t2 * t, u = 1.0 - t;
  w[0] = u * u * u / 6.0;
  w[1] = (3.0 * t3 - 6.0 * t2 + 4.0) / 6.0;
  w[2] = (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0;
  w[3] = t3 / 6.0;
}

__global__ __launch_bounds__(PREP_THREADS) void k_prep_resample_cubic(CubicParams p) {
  const unsigned gw = (p.OW + 3) / 4, total = p.N * p.OD * p.OH * gw;
  for (unsigned e = blockIdx.x * PREP_THREADS + threadIdx.x; e < total; e += gridDim.x * PREP_THREADS) {
    const RowItem r = row_item(e, gw, p.OD, p.OH);
    unsigned id[4], ih[4], d0, d1, h0, h1;
    double wd[4], wh[4];
    cubic_axis(r.d, p.fd, p.D, id, wd, d0, d1);
    cubic_axis(r.h, p.fh, p.H, ih, wh, h0, h1);
    const size_t plane = (size_t)r.n * p.D;
    float out[4];
#pragma unroll
    for (unsigned u = 0; u < 4; ++u) {
      const unsigned ow = min(r.w0 + u, p.OW - 1);
      unsigned iw[4], w0, w1;
      double ww[4];
      cubic_axis(ow, p.fw, p.W, iw, ww, w0, w1);
      // w innermost, then h, then d: row sums, plane sums, the voxel
      double acc = 0.0;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        double pl = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double* __restrict__ row = p.c + ((plane + id[a]) * p.H + ih[b]) * p.W;
          double rs = ww[0] * row[iw[0]];
          rs += ww[1] * row[iw[1]];
          rs += ww[2] * row[iw[2]];
          rs += ww[3] * row[iw[3]];
          pl = b == 0 ? wh[0] * rs : pl + wh[b] * rs;
        }
        acc = a == 0 ? wd[0] * pl : acc + wd[a] * pl;
      }
      float v = (float)acc;
      if (p.zero_keep) {
        const float* __restrict__ r00 = p.x + ((plane + d0) * p.H + h0) * p.W;
        const float* __restrict__ r01 = p.x + ((plane + d0) * p.H + h1) * p.W;
        const float* __restrict__ r10 = p.x + ((plane + d1) * p.H + h0) * p.W;
        const float* __restrict__ r11 = p.x + ((plane + d1) * p.H + h1) * p.W;
        const bool zero = r00[w0] == 0.0f && r00[w1] == 0.0f && r01[w0] == 0.0f && r01[w1] == 0.0f &&
                          r10[w0] == 0.0f && r10[w1] == 0.0f && r11[w0] == 0.0f && r11[w1] == 0.0f;      // a NaN is not
        v = zero ? 0.0f : v;
      }
      out[u] = v;
    }
    float* dst = p.y + (((size_t)r.n * p.OD + r.d) * p.OH + r.h) * p.OW + r.w0;
    if (r.w0 + 4 <= p.OW) {
      PFloat4 o;
      o.x = out[0]; o.y = out[1]; o.z = out[2]; o.w = out[3];
      *reinterpret_cast<PFloat4*>(dst) = o;
    } else {
      for (unsigned u = 0; r.w0 + u < p.OW; ++u) dst[u] = out[u];
    }
  }
}

// the work items of the four launches for a shape: lines of the D and H passes, rows of the W pass (0: not launched),
// items of four output voxels of the evaluation
struct CubicItems {
  size_t d, h, w, eval;
};
static inline CubicItems cubic_items(int N, int D, int H, int W, int OD, int OH, int OW) {
  CubicItems it;
  it.d = (size_t)N * H * W;
  it.h = H > 1 ? (size_t)N * D * W : 0;
  it.w = W > 1 ? (size_t)N * D * H : 0;
  it.eval = (size_t)N * OD * OH * ((OW + 3) / 4);
  return it;
}

// the capped grid of the W pass: one workgroup per tile of SPL_ROWS rows
static inline unsigned spline_w_grid(size_t rows) { return prep_grid(rows * (PREP_THREADS / SPL_ROWS)); }

static int launch_prefilter(const float* x, int N, int D, int H, int W, int passes, double* ws, hipStream_t st) {
  const CubicItems it = cubic_items(N, D, H, W, 1, 1, 1);
  const dim3 t(PREP_THREADS);
  LineParams p;
  p.ws = ws;
  if (passes & EFFQ_PREP_SPLINE_PASS_D) {
    p.src = x; p.lines = (unsigned)it.d; p.ext = D; p.stride = (unsigned)H * W;
    hipLaunchKernelGGL(k_prep_spline_lines<float>, dim3(prep_grid(it.d)), t, 0, st, p);
    EFFQ_LAUNCH_CHECK();
  }
  if ((passes & EFFQ_PREP_SPLINE_PASS_H) && it.h) {
    p.src = ws; p.lines = (unsigned)it.h; p.ext = H; p.stride = W;
    hipLaunchKernelGGL(k_prep_spline_lines<double>, dim3(prep_grid(it.h)), t, 0, st, p);
    EFFQ_LAUNCH_CHECK();
  }
  if ((passes & EFFQ_PREP_SPLINE_PASS_W) && it.w) {
    hipLaunchKernelGGL(k_prep_spline_w, dim3(spline_w_grid(it.w)), t, 0, st, ws, (unsigned)it.w, (unsigned)W);
    EFFQ_LAUNCH_CHECK();
  }
  return EFFQ_OK;
}

static inline size_t cubic_ws_bytes(int N, int D, int H, int W) { return (size_t)N * D * H * W * sizeof(double); }
static inline bool factor_ok(double f) { return f > 0.0 && f <= 1e6; }      // false for a NaN

}  // namespace effq
using namespace effq;

extern "C" {

int effq_prep_cubic_ws_bytes(int N, int D, int H, int W, size_t* bytes) {
  EFFQ_CHECK_ARG(bytes && prep_fits(N, D, H, W));
  *bytes = cubic_ws_bytes(N, D, H, W);
  return EFFQ_OK;
}

int effq_prep_cubic_plan(int N, int D, int H, int W, int OD, int OH, int OW, int* chunk, int* tile_rows, long long* items,
                         long long* trip) {
  EFFQ_CHECK_ARG(chunk && tile_rows && items && trip && prep_fits(N, D, H, W) && prep_fits(N, OD, OH, OW));
  *chunk = SPL_CHUNK;
  *tile_rows = SPL_ROWS;
  const CubicItems it = cubic_items(N, D, H, W, OD, OH, OW);
  const size_t n[4] = {it.d, it.h, it.w, it.eval};
  for (int k = 0; k < 4; ++k) {
    items[k] = (long long)n[k];
    trip[k] = n[k] ? (long long)prep_grid(n[k]) * PREP_THREADS : 0;      // one thread per line or item
  }
  if (it.w) trip[2] = (long long)spline_w_grid(it.w) * SPL_ROWS;           // one workgroup per tile
  return EFFQ_OK;
}

int effq_prep_spline_prefilter(const float* x, int N, int D, int H, int W, int passes, void* ws, size_t ws_bytes,
                               void* stream) {
  EFFQ_CHECK_ARG(ws && prep_fits(N, D, H, W) && aligned_to(ws, 8) && ws_bytes >= cubic_ws_bytes(N, D, H, W));
  EFFQ_CHECK_ARG(passes > 0 && passes <= 7);
  EFFQ_CHECK_ARG(!(passes & EFFQ_PREP_SPLINE_PASS_D) || (x && aligned_to(x, 4)));
  return launch_prefilter(x, N, D, H, W, passes, static_cast<double*>(ws), as_stream(stream));
}

int effq_prep_resample_cubic(const float* x, int N, int D, int H, int W, double fd, double fh, double fw, int zero_keep,
                             float* y, int OD, int OH, int OW, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(x && y && ws && prep_fits(N, D, H, W) && prep_fits(N, OD, OH, OW));
  EFFQ_CHECK_ARG(aligned_to(x, 4) && aligned_to(y, 4) && aligned_to(ws, 8));
  EFFQ_CHECK_ARG(ws_bytes >= cubic_ws_bytes(N, D, H, W));
  EFFQ_CHECK_ARG(factor_ok(fd) && factor_ok(fh) && factor_ok(fw) && (zero_keep == 0 || zero_keep == 1));
  const hipStream_t st = as_stream(stream);
  const int rc = launch_prefilter(x, N, D, H, W, 7, static_cast<double*>(ws), st);
  if (rc != EFFQ_OK) return rc;
  CubicParams p;
  p.x = x; p.c = static_cast<const double*>(ws); p.y = y;
  p.N = N; p.D = D; p.H = H; p.W = W; p.OD = OD; p.OH = OH; p.OW = OW;
  p.fd = fd; p.fh = fh; p.fw = fw; p.zero_keep = zero_keep;
  hipLaunchKernelGGL(k_prep_resample_cubic, dim3(prep_grid(cubic_items(N, D, H, W, OD, OH, OW).eval)), dim3(PREP_THREADS), 0,
                     st, p);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
