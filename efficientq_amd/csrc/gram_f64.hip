// effq_gram_f64: the UNWEIGHTED Gram system of a layer with a full-precision input, in fp64 on the matrix cores:
//     Au = sum_v xhat_v xhat_v^T  (n x n),   Bu = sum_v y_v xhat_v^T  (c2 x n),   xhat_v = [im2col patch of x; 1].
// These are the operands of effq_gram_loss (gram_loss.hip): with them the 200 per-iteration losses of a layer
// (F.mse_loss(F.conv3d(x, G, b*), y), EfficientQConv.py:118-122) cost c2 n^2 multiply-adds each instead of a pass over
// all calibration voxels.  The layers with QUANTISED input get Au / Bu from the exact-integer Gram pass
// (effq_gram_accum_i8_unw); the first conv and the classifier (q_first = q_last = "256,-1": full-precision activations,
// quirk Q14) have no level ids, so their system is accumulated here - fp32 values widened to fp64, products exact
// (24 + 24 bits), fp64 accumulation on v_mfma_f64_16x16x4_f64.  n <= 128 (first conv 4 -> 32, 3^3: n = 109; classifier
// 32 -> 3, 1^3: n = 33; LiTS first conv: n = 28), c2 <= 64.
// Patch order = the reference's im2col row order (c1, kd, kh, kw) (solver.py:104-108), voxel order (n, d, h, w).
// Persistent workgroups; every workgroup keeps its accumulator tiles in registers over all its voxel chunks and writes
// ONE partial slab at the end; a second kernel adds the slabs in workgroup order (deterministic) and mirrors Au.
// The gather is pipelined where the layer allows it (k_gram_f64<TPW, true>: C1 % 4 == 0, x and y 16-byte aligned, at most
// GF_NX 16-byte cells of x and one cell or value of y per thread and chunk - the first conv and the classifier): the cells
// of the NEXT chunk are loaded into registers in front of the matrix-core loop and stored to LDS behind it.  Both forms
// stage the same LDS rows, so the results do not depend on the form.
#include "common.h"

namespace effq {

typedef double f64x4g __attribute__((ext_vector_type(4)));

constexpr int GF_VC = 32;            // voxels per LDS chunk
constexpr int GF_T = 256;
constexpr int GF_MAXN = 128, GF_MAXC2 = 64;
constexpr int GF_MAXTILES = 72;      // 36 (upper triangle at 8 tiles per edge) + 32 (4 x 8) rounded up
constexpr int GF_NX = 4;             // 16-byte cells of x a thread of the pipelined gather holds

struct GramF64Params {
  const float* x;                    // NDHWC
  const float* y;                    // NDHWC (output voxels x c2)
  effq_geom g;
  int n, has_bias, np, c2p, ld;      // np = n rounded up to 16, row = [np patch entries | c2p target entries | pad]
  int od, oh, ow;
  long long V;                       // output voxels
  int nchunk, ntiles, te, tc;        // te = np / 16, tc = c2p / 16
  double* slab;                      // [gridDim.x][ntiles][256]
  int vecy;                          // pipelined gather: y by 16-byte cells (C2 % 4 == 0), else by values
  int step[4];                       // ... gridDim.x * GF_VC output voxels as (n, od, oh, ow) steps
};

template <int TPW, bool PIPE>
__global__ __launch_bounds__(GF_T, (TPW <= 3 || (TPW <= 6 && !PIPE)) ? 4 : 2) void k_gram_f64(GramF64Params p) {
  extern __shared__ __attribute__((aligned(16))) double rows[];      // [GF_VC][ld]
  __shared__ int tab_a[GF_MAXTILES], tab_b[GF_MAXTILES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  // tile table: Au tiles (ti <= tj) then Bu tiles; entry = column offset of the A / B operand inside a row
  if (tid == 0) {
    int t = 0;
    for (int i = 0; i < p.te; ++i)
      for (int j = i; j < p.te; ++j) {
        tab_a[t] = 16 * i;
        tab_b[t] = 16 * j;
        ++t;
      }
    for (int c = 0; c < p.tc; ++c)
      for (int j = 0; j < p.te; ++j) {
        tab_a[t] = p.np + 16 * c;
        tab_b[t] = 16 * j;
        ++t;
      }
  }
  __syncthreads();
  int aoff[TPW], boff[TPW];
  f64x4g acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tile = wid + 4 * t;
    const bool ok = tile < p.ntiles;
    aoff[t] = ok ? tab_a[tile] : 0;
    boff[t] = ok ? tab_b[tile] : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = 0.0;
  }
  const int nw = p.n - p.has_bias;
  const int k3 = p.g.KD * p.g.KH * p.g.KW, k2 = p.g.KH * p.g.KW;
  const int V = (int)p.V;
  constexpr int KUNROLL = PIPE ? 1 : 2;                // the registers of a second step go to the prefetched cells
  auto consume = [&]() {                               // one chunk of LDS rows through the matrix cores
#pragma unroll KUNROLL
    for (int ks = 0; ks < GF_VC / 4; ++ks) {
      const double* r0 = rows + (ks * 4 + lk) * p.ld + lr;
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const double a = r0[aoff[t]], b = r0[boff[t]];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
      }
    }
  };
  if constexpr (!PIPE) {
  // patch-entry table (c, kd, kh, kw) of the reference's im2col row order, decoded once
  __shared__ int qtab[GF_MAXN];
  __shared__ int vrow[GF_VC][4];                       // per chunk row: batch index and input origin (id0, ih0, iw0)
  {
    for (int q = tid; q < nw; q += GF_T) {
      const int c = q / k3, kr = q - c * k3;
      const int kd = kr / k2, kr2 = kr - kd * k2;
      const int kh = kr2 / p.g.KW, kw = kr2 - kh * p.g.KW;
      qtab[q] = c | (kd << 16) | (kh << 20) | (kw << 24);
    }
  }
  const int rowlen = p.np + p.c2p;
  for (int ch = blockIdx.x; ch < p.nchunk; ch += gridDim.x) {
    __syncthreads();                                   // the previous chunk has been consumed (and qtab is written)
    const int v0 = ch * GF_VC;
    if (tid < GF_VC) {
      const int v = v0 + tid;
      int t = v;
      const int ow_ = t % p.ow;
      t /= p.ow;
      const int oh_ = t % p.oh;
      t /= p.oh;
      const int od_ = t % p.od;
      vrow[tid][0] = (v < V) ? t / p.od : -1;
      vrow[tid][1] = od_ * p.g.SD - p.g.PD;
      vrow[tid][2] = oh_ * p.g.SH - p.g.PH;
      vrow[tid][3] = ow_ * p.g.SW - p.g.PW;
    }
    __syncthreads();
    for (int e = tid; e < GF_VC * rowlen; e += GF_T) {
      const int vl = e / rowlen, q = e - vl * rowlen;
      const int nn = vrow[vl][0];
      double val = 0.0;
      if (nn >= 0) {
        if (q < nw) {
          const int pk = qtab[q];
          const int c = pk & 0xffff;
          const int id = vrow[vl][1] + ((pk >> 16) & 15), ih = vrow[vl][2] + ((pk >> 20) & 15),
                    iw = vrow[vl][3] + ((pk >> 24) & 15);
          if (id >= 0 && id < p.g.D && ih >= 0 && ih < p.g.H && iw >= 0 && iw < p.g.W)
            val = (double)p.x[((((size_t)nn * p.g.D + id) * p.g.H + ih) * p.g.W + iw) * p.g.C1 + c];
        } else if (q < p.n) {
          val = 1.0;                                   // the ones row of the bias column (solver.py:256)
        } else if (q >= p.np && q - p.np < p.g.C2) {
          val = (double)p.y[(size_t)(v0 + vl) * p.g.C2 + (q - p.np)];
        }
      }
      rows[vl * p.ld + q] = val;
    }
    __syncthreads();
    consume();
  }
  } else {
  // Every thread holds up to GF_NX 16-byte cells of x (the 4 channels of one tap: 4 rows of the (c, kd, kh, kw) order) and
  // one cell or value of y of the NEXT chunk in registers.  The loads are unconditional on clamped addresses and masked
  // where they are stored.  A thread's cells keep their chunk row, tap and channels from chunk to chunk, and the output
  // voxel of a cell advances by the same gridDim.x * GF_VC voxels every time: its coordinates (n, od, oh, ow) are carried
  // along by a mixed-radix addition (p.step) - no division inside the loop, whose integer work would otherwise cost as
  // much as the matrix cores'.
  const int c4x = p.g.C1 >> 2, perx = k3 * c4x, nx = GF_VC * perx;
  const int ycell = p.vecy ? (p.g.C2 >> 2) : p.g.C2, ny = GF_VC * ycell;
  const int ncell = (nx + GF_T - 1) / GF_T;            // <= GF_NX
  int xkd[GF_NX], xkh[GF_NX], xkw[GF_NX], xc[GF_NX], xd[GF_NX];   // per cell: tap (minus padding), first channel, LDS offset
  int vn[GF_NX], vd[GF_NX], vh[GF_NX], vw[GF_NX];                 // ... and the output voxel of the chunk being prefetched
  float4 px[GF_NX], py = make_float4(0.f, 0.f, 0.f, 0.f);
  bool okx[GF_NX], oky = false;
#pragma unroll
  for (int i = 0; i < GF_NX; ++i) {
    const int e = min(tid + i * GF_T, nx - 1);
    const int vl = e / perx, r = e - vl * perx;
    const int tap = r / c4x, c4 = r - tap * c4x;
    const int kd = tap / k2, kr2 = tap - kd * k2, kh = kr2 / p.g.KW;
    xkd[i] = kd - p.g.PD;
    xkh[i] = kh - p.g.PH;
    xkw[i] = kr2 - kh * p.g.KW - p.g.PW;
    xc[i] = 4 * c4;
    xd[i] = vl * p.ld + 4 * c4 * k3 + tap;
    int t = blockIdx.x * GF_VC + vl;                   // < V + GF_VC < 2^31; n >= N marks a voxel past the end
    vw[i] = t % p.ow;
    t /= p.ow;
    vh[i] = t % p.oh;
    t /= p.oh;
    vd[i] = t % p.od;
    vn[i] = t / p.od;
    px[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    okx[i] = false;
  }
  const int ye = min(tid, ny - 1), yl = ye / ycell, yc = (ye - yl * ycell) * (p.vecy ? 4 : 1);
  // x of the chunks blockIdx.x, blockIdx.x + gridDim.x, ... in turn (the carried coordinates), y of chunk ch
  auto prefetch = [&](int ch) {
#pragma unroll
    for (int i = 0; i < GF_NX; ++i)
      if (i < ncell) {
        const int id = vd[i] * p.g.SD + xkd[i], ih = vh[i] * p.g.SH + xkh[i], iw = vw[i] * p.g.SW + xkw[i];
        okx[i] = vn[i] < p.g.N && id >= 0 && id < p.g.D && ih >= 0 && ih < p.g.H && iw >= 0 && iw < p.g.W;
        const int cn = min(vn[i], p.g.N - 1), cd = min(max(id, 0), p.g.D - 1), chh = min(max(ih, 0), p.g.H - 1),
                  cw = min(max(iw, 0), p.g.W - 1);
        px[i] = *reinterpret_cast<const float4*>(
            p.x + ((((size_t)cn * p.g.D + cd) * p.g.H + chh) * p.g.W + cw) * p.g.C1 + xc[i]);
        int c;                                         // the voxel of the next call
        vw[i] += p.step[3];
        c = vw[i] >= p.ow;
        vw[i] -= c ? p.ow : 0;
        vh[i] += p.step[2] + c;
        c = vh[i] >= p.oh;
        vh[i] -= c ? p.oh : 0;
        vd[i] += p.step[1] + c;
        c = vd[i] >= p.od;
        vd[i] -= c ? p.od : 0;
        vn[i] = min(vn[i] + p.step[0] + c, p.g.N);
      }
    const int v = ch * GF_VC + yl;
    oky = v < V;
    const float* src = p.y + (size_t)(oky ? v : 0) * p.g.C2 + yc;
    if (p.vecy)
      py = *reinterpret_cast<const float4*>(src);
    else
      py.x = *src;
  };
  // the padding of the patch entries and of the targets holds no value: zero once
  {
    const int t0 = p.np - p.n, trest = t0 + p.c2p - p.g.C2;
    for (int e = tid; e < GF_VC * trest; e += GF_T) {
      const int vl = e / trest, r = e - vl * trest;
      rows[vl * p.ld + (r < t0 ? p.n + r : p.np + p.g.C2 + (r - t0))] = 0.0;
    }
  }
  auto stage = [&](int ch) {
#pragma unroll
    for (int i = 0; i < GF_NX; ++i)
      if (tid + i * GF_T < nx) {
        const float4 val = okx[i] ? px[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        double* d = rows + xd[i];
        d[0] = (double)val.x;
        d[k3] = (double)val.y;
        d[2 * k3] = (double)val.z;
        d[3 * k3] = (double)val.w;
      }
    if (tid < ny) {
      const float4 val = oky ? py : make_float4(0.f, 0.f, 0.f, 0.f);
      double* d = rows + yl * p.ld + p.np + yc;
      d[0] = (double)val.x;
      if (p.vecy) {
        d[1] = (double)val.y;
        d[2] = (double)val.z;
        d[3] = (double)val.w;
      }
    }
    if (p.has_bias && tid < GF_VC) rows[tid * p.ld + nw] = (ch * GF_VC + tid < V) ? 1.0 : 0.0;   // the ones row (solver.py:256)
  };
  prefetch(blockIdx.x);
  for (int ch = blockIdx.x; ch < p.nchunk; ch += gridDim.x) {
    __syncthreads();                                   // the previous chunk has been consumed
    stage(ch);
    __syncthreads();
    const int next = ch + gridDim.x;
    prefetch(next < p.nchunk ? next : ch);             // unconditional: after the last chunk no x is valid, y is read again
    consume();
  }
  }
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tile = wid + 4 * t;
    if (tile < p.ntiles) {
      double* dst = p.slab + ((size_t)blockIdx.x * p.ntiles + tile) * 256;
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[r * 64 + lane] = acc[t][r];
    }
  }
}

// Au / Bu = sum of the slabs in workgroup order; element (r, lane) of a tile is (row = lane / 16 + 4 r, col = lane % 16)
__global__ __launch_bounds__(256) void k_gram_f64_reduce(GramF64Params p, int nslab, double* __restrict__ Au,
                                                         double* __restrict__ Bu) {
  const int tile = blockIdx.x, e = threadIdx.x;
  const double* src = p.slab + (size_t)tile * 256 + e;
  const size_t stride = (size_t)p.ntiles * 256;
  double s = 0.0;
  int w = 0;
  for (; w + 16 <= nslab; w += 16) {                   // 16 loads in flight, the additions in workgroup order
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = src[(size_t)(w + k) * stride];
#pragma unroll
    for (int k = 0; k < 16; ++k) s += v[k];
  }
  for (; w < nslab; ++w) s += src[(size_t)w * stride];
  const int r = e >> 6, lane = e & 63;
  const int row = (lane >> 4) + 4 * r, col = lane & 15;
  const int nau = p.te * (p.te + 1) / 2;
  if (tile < nau) {
    int i = 0, rem = tile;
    while (rem >= p.te - i) {
      rem -= p.te - i;
      ++i;
    }
    const int j = i + rem;
    const int gi = 16 * i + row, gj = 16 * j + col;
    if (gi < p.n && gj < p.n) {
      Au[(size_t)gi * p.n + gj] = s;
      if (i != j) Au[(size_t)gj * p.n + gi] = s;     // mirror of an off-diagonal tile (diagonal tiles hold both halves)
    }
  } else {
    const int t = tile - nau;
    const int c = t / p.te, j = t - c * p.te;
    const int gc = 16 * c + row, gj = 16 * j + col;
    if (gc < p.g.C2 && gj < p.n) Bu[(size_t)gc * p.n + gj] = s;
  }
}

static bool gram_f64_plan(const effq_geom* g, int has_bias, GramF64Params* p) {
  if (g == nullptr) return false;
  const long long nw = (long long)g->C1 * g->KD * g->KH * g->KW;
  const long long n = nw + (has_bias ? 1 : 0);
  if (n < 1 || n > GF_MAXN || g->C2 < 1 || g->C2 > GF_MAXC2) return false;
  const int od = (g->D + 2 * g->PD - g->KD) / g->SD + 1, oh = (g->H + 2 * g->PH - g->KH) / g->SH + 1,
            ow = (g->W + 2 * g->PW - g->KW) / g->SW + 1;
  if (od <= 0 || oh <= 0 || ow <= 0 || g->N <= 0) return false;
  p->g = *g;
  p->n = (int)n;
  p->has_bias = has_bias ? 1 : 0;
  p->np = ((int)n + 15) / 16 * 16;
  p->c2p = (g->C2 + 15) / 16 * 16;
  p->ld = p->np + p->c2p + 2;                       // (+2 doubles: rows of 16-double operand reads land on shifted banks)
  p->od = od; p->oh = oh; p->ow = ow;
  p->V = (long long)g->N * od * oh * ow;
  p->nchunk = (int)((p->V + GF_VC - 1) / GF_VC);
  p->te = p->np / 16;
  p->tc = p->c2p / 16;
  p->ntiles = p->te * (p->te + 1) / 2 + p->tc * p->te;
  return p->ntiles <= GF_MAXTILES && p->V < ((long long)1 << 31) - GF_VC && g->KD <= 15 && g->KH <= 15 && g->KW <= 15;
}

// persistent grid: 4 workgroups per CU (37 KB of LDS and <= 128 registers each): the gather of the patches is a stream of
// 4-byte loads that only many waves in flight keep busy (one workgroup per CU: 10.4 ms for the first conv of the BraTS
// net, 11 % of the fp64 matrix peak)
static int gram_f64_grid(const GramF64Params& p) { return p.nchunk < 1024 ? p.nchunk : 1024; }

// accumulator tiles per wave the kernel is instantiated for: the smallest of 3 / 6 / 11 / 18 that holds ceil(ntiles / 4)
static int gram_f64_tpw(const GramF64Params& p) {
  const int tpw = (p.ntiles + 3) / 4;
  return tpw <= 3 ? 3 : (tpw <= 6 ? 6 : (tpw <= 11 ? 11 : 18));
}

// the pipelined gather: x by 16-byte cells, at most GF_NX of them and one cell (or value) of y per thread and chunk
static bool gram_f64_pipe(const GramF64Params& p, const void* x, const void* y, int* vecy) {
  const effq_geom& g = p.g;
  if ((g.C1 & 3) != 0 || (reinterpret_cast<uintptr_t>(x) & 15) != 0) return false;
  *vecy = ((g.C2 & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0) ? 1 : 0;
  const int xcells = GF_VC * (p.n - p.has_bias) / 4, ycells = GF_VC * (*vecy ? g.C2 / 4 : g.C2);
  return xcells <= GF_NX * GF_T && ycells <= GF_T && gram_f64_tpw(p) <= 11;      // 18 tiles leave no registers for it
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_gram_f64_supported(const effq_geom* g, int has_bias) {
  GramF64Params p;
  return gram_f64_plan(g, has_bias, &p) ? 1 : 0;
}

size_t effq_gram_f64_ws_bytes(const effq_geom* g, int has_bias) {
  GramF64Params p;
  if (!gram_f64_plan(g, has_bias, &p)) return 0;
  return (size_t)gram_f64_grid(p) * p.ntiles * 256 * sizeof(double);
}

int effq_gram_f64(const float* x_ndhwc, const float* y_ndhwc, const effq_geom* g, int has_bias, double* Au, double* Bu,
                  void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(x_ndhwc && y_ndhwc && g && Au && Bu && ws);
  GramF64Params p;
  if (!gram_f64_plan(g, has_bias, &p)) {
    set_error("gram_f64: unsupported geometry (n = C1*k^3 + bias <= %d, C2 <= %d)", GF_MAXN, GF_MAXC2);
    return EFFQ_ERR_ARG;
  }
  const size_t need = effq_gram_f64_ws_bytes(g, has_bias);
  if (ws_bytes < need) {
    set_error("gram_f64: workspace %zu < required %zu", ws_bytes, need);
    return EFFQ_ERR_WORKSPACE;
  }
  p.x = x_ndhwc;
  p.y = y_ndhwc;
  p.slab = reinterpret_cast<double*>(ws);
  const int grid = gram_f64_grid(p);
  const size_t lds = (size_t)GF_VC * p.ld * sizeof(double);
  hipStream_t st = as_stream(stream);
  p.vecy = 0;
  const bool pipe = gram_f64_pipe(p, x_ndhwc, y_ndhwc, &p.vecy);
  {
    long long t = (long long)grid * GF_VC;
    p.step[3] = (int)(t % p.ow);
    t /= p.ow;
    p.step[2] = (int)(t % p.oh);
    t /= p.oh;
    p.step[1] = (int)(t % p.od);
    p.step[0] = (int)(t / p.od);
  }
#define EFFQ_GF(TPW_, PIPE_) hipLaunchKernelGGL((k_gram_f64<TPW_, PIPE_>), dim3(grid), dim3(GF_T), lds, st, p)
  switch (gram_f64_tpw(p)) {
    case 3: if (pipe) EFFQ_GF(3, true); else EFFQ_GF(3, false); break;
    case 6: if (pipe) EFFQ_GF(6, true); else EFFQ_GF(6, false); break;
    case 11: if (pipe) EFFQ_GF(11, true); else EFFQ_GF(11, false); break;
    default: EFFQ_GF(18, false); break;
  }
#undef EFFQ_GF
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gram_f64_reduce, dim3(p.ntiles), dim3(256), 0, st, p, grid, Au, Bu);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// the launch effq_gram_f64 makes for a geometry (launches nothing): the same gram_f64_plan, _grid and _tpw
int effq_gram_f64_plan_query(const effq_geom* g, int has_bias, int* nchunk, int* grid, int* ntiles, int* tpw) {
  EFFQ_CHECK_ARG(g && nchunk && grid && ntiles && tpw);
  GramF64Params p;
  EFFQ_CHECK_ARG(gram_f64_plan(g, has_bias, &p));
  *nchunk = p.nchunk;
  *grid = gram_f64_grid(p);
  *ntiles = p.ntiles;
  *tpw = gram_f64_tpw(p);
  return EFFQ_OK;
}

// 1 where effq_gram_f64 gathers these inputs with the pipelined loop, 0 where with the plain one (launches nothing)
int effq_gram_f64_pipelined(const float* x_ndhwc, const float* y_ndhwc, const effq_geom* g, int has_bias) {
  GramF64Params p;
  int vecy = 0;
  return (gram_f64_plan(g, has_bias, &p) && gram_f64_pipe(p, x_ndhwc, y_ndhwc, &vecy)) ? 1 : 0;
}

}  // extern "C"
