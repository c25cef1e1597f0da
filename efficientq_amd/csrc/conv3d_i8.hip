// conv3d_calib_step_i8: the "int-simulated" fake-quant forward of one ADMM iteration, exact.
// Reference: EfficientQConv.py:118-122 (conv3d(Qactivation, G, b*) + mse_loss, 200x per layer).
//
// With quantised activations x = alpha_a * k/(La-1) (k = level id >= 0) and projected weights
// G = alpha_w * j'/(Lw-1) (j' = 2*level - (Lw-1)), the conv is  s * sum k*j'  with small integers, so it
// runs on the i8 matrix cores with exact int32 accumulation (v_mfma_i32_32x32x32_i8: K = 32 channels
// per instruction, 32x the f32 MFMA rate) and one fp32 scale + bias in the epilogue.  The kernel is
// then HBM-bound: per output voxel it streams C2*4 bytes of target and C1 bytes of level ids.
//
// Mapping: persistent workgroups (4 waves) walk contiguous runs of 4x4x8 output tiles; wave w owns
// d-plane w (32 voxels) x 32 output channels.  The wave's B operands -- all 27 taps x C1/32 channel
// groups of its 32 output channels -- live in REGISTERS for the whole kernel (27*CG*4 VGPRs), the
// level-id halo tile (6x6x10 voxels x C1 bytes) is staged through LDS with a 16-byte pad per voxel,
// and the next tile's halo + targets are prefetched into registers under the current tile's MFMAs.
//
// Layout of this file: the weight packs; the shared stages (TileLayout, tile run and decode, halo slots / prefetch / commit,
// A fragment offsets, targets and epilogues in both layouts, the two tile loops), each written once per form; the seven
// kernels, which add where their B operands live and their MFMA loop; the host plan and launches.  DESIGN.md section 4 lists
// which kernel takes which form, and the two kernels that keep code of their own.
#include <stdlib.h>
#include "common.h"

namespace effq {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

typedef float yv4 __attribute__((ext_vector_type(4)));

constexpr int ITH = 4, ITW = 8;                       // every tile is 4 x 8 output voxels in (h, w); its depth varies
constexpr int I_HH = ITH + 2, I_HW = ITW + 2;
// Halo tile in LDS: voxel (row, col) of a row of I_HW voxels sits at row * (I_HW * VS + pad) + col * VS.  A wave reads
// A fragments with lane -> (h = lane >> 3 & 3, w = lane & 7); ds_read_b128 is served in the lane groups {0-3, 12-15,
// 20-27} / {4-11, 16-19, 28-31} (MI355X_MICROARCH.md, LDS): with rows packed back to back (pad 0) three lanes of a
// group shared a bank quad at every channel count (SQ_LDS_BANK_CONFLICT = 56 % of SQ_LDS_IDX_ACTIVE on k_conv3d_i8l2),
// the pads below spread the 16 lanes of each group over all 64 banks.
__host__ __device__ constexpr int halo_row_pad(int cg) { return cg == 1 ? 160 : cg == 2 ? 96 : 224; }

struct ConvI8Params {
  const int8_t* x;
  const int8_t* wq;
  const float* bias;
  const float* y;
  const float* act_alpha;
  const effq_fp_state* wstate;
  double inv_levels;
  int N, C1, C2, c2p, D, H, W, OD, OH, OW, PD, PH, PW;
  int tiles_d, tiles_h, tiles_w, ntiles;
  double* partials;
  unsigned int* ticket;
  double* sqerr;
  // conv3d_quant_forward_i8 (k_conv3d_i8l2e<true>, k_conv3d_i8w<true>): the conv output is also STORED (fp32, NDHWC) and
  // sqerr[1] is the attention-weighted sum (att: one weight per output voxel, or NULL = the plain sum once more)
  float* out;
  const float* att;
};

__global__ __launch_bounds__(256) void k_pack_weight_i8(const int8_t* __restrict__ Gq, int8_t* __restrict__ wq, int C1,
                                                        int C2, int T, int c2p) {
  const size_t total = (size_t)T * c2p * C1;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const int c = (int)(e % C1);
    size_t r = e / C1;
    const int j = (int)(r % c2p);
    const int tap = (int)(r / c2p);
    wq[e] = (j < C2) ? Gq[((size_t)j * C1 + c) * T + tap] : (int8_t)0;
  }
}

// Packed layout for the wide-channel kernel: [tap][group g][k-half h][c2p][16 bytes], so that the B operand of one
// MFMA is a 512-byte contiguous run per lane half (coalesced 16-byte loads straight from L2).
template <int RPW>      // output channels per workgroup: 4 = 64-byte store runs, 1 = four times as many workgroups
__global__ __launch_bounds__(256) void k_pack_weight_i8g(const int8_t* __restrict__ Gq, int8_t* __restrict__ wq, int C1,
                                                         int C2, int T, int c2p) {
  // One workgroup = RPW output channels: their rows of Gq ([C1][T] bytes each, contiguous) are read coalesced into LDS,
  // then every thread assembles 16-byte cells (tap, g, h, j) from bytes T apart in LDS and stores them - with RPW = 4 the
  // 4 channels of a (tap, g, h) are 64 contiguous bytes.  (One thread per cell gathering its 16 bytes from global memory,
  // T bytes apart, took 43-69 us per call in situ for 1.77 MB of weights.)
  extern __shared__ __attribute__((aligned(16))) int8_t rows[];          // [RPW][C1 * T]
  const int rowb = C1 * T;
  const int j0 = blockIdx.x * RPW;
  const int rowv = rowb / 16;                      // C1 % 16 == 0: rows are whole 16-byte vectors
  for (int e = threadIdx.x; e < RPW * rowv; e += 256) {
    const int jj = e / rowv, o = e - jj * rowv;
    v4i val = {0, 0, 0, 0};
    if (j0 + jj < C2) val = *reinterpret_cast<const v4i*>(Gq + (size_t)(j0 + jj) * rowb + (size_t)o * 16);
    *reinterpret_cast<v4i*>(rows + (size_t)jj * rowb + (size_t)o * 16) = val;
  }
  __syncthreads();
  const int ncell = T * (C1 / 16);                                       // cells per output channel
  for (int u = threadIdx.x; u < ncell * RPW; u += 256) {
    const int jj = u % RPW, q = u / RPW;
    const int gh = q % (C1 / 16), tap = q / (C1 / 16);
    if (j0 + jj >= c2p) continue;
    const int8_t* src = rows + jj * rowb + (16 * gh) * T + tap;
    v4i out;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      unsigned wv = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) wv |= (unsigned)(unsigned char)src[(4 * w + b) * T] << (8 * b);
      out[w] = (int)wv;
    }
    *reinterpret_cast<v4i*>(wq + ((size_t)(tap * (C1 / 16) + gh) * c2p + j0 + jj) * 16) = out;
  }
}

// ======================================================================================================================
// Shared stages of the persistent conv kernels.  Each stage is written once per form; a kernel is its TileLayout, the
// composition of stages in one of the two tile loops below, and its own part: where its B operands live and its MFMA loop.
// ======================================================================================================================

// A workgroup's tile and everything that follows from its three numbers: THREADS per workgroup, tile depth TD (the
// tile is TD x 4 x 8 output voxels) and CG groups of 32 input channels.
template <int THREADS_, int TD_, int CG_>
struct TileLayout {
  static constexpr int THREADS = THREADS_, TD = TD_, CG = CG_, C1 = 32 * CG;
  static constexpr int HD = TD + 2, NVOX = HD * I_HH * I_HW;         // halo voxels
  static constexpr int PARTS = 2 * CG, NSLOT = NVOX * PARTS;         // 16-byte parts per voxel / slots per tile
  static constexpr int NHL = (NSLOT + THREADS - 1) / THREADS;        // halo 16-byte loads per thread
  static constexpr int VS = 32 * CG + 16;                            // bytes per halo voxel in LDS (16-byte pad)
  static constexpr int PADB = halo_row_pad(CG), ROWB = I_HW * VS + PADB;
  static constexpr int HALOB = HD * I_HH * ROWB, HALOB16 = (HALOB + 15) / 16 * 16;
  // wave -> (plane, channel half): WPL waves side by side over the d-planes, each NPL planes deep (plane, plane + 4);
  // the remaining waves take further halves of 32 output channels: NCH output channels per workgroup
  static constexpr int WPL = TD < 4 ? TD : 4, NPL = TD / WPL, NCH = 32 * (THREADS / 64 / WPL);
  // transposed epilogue: rows of NCH floats + pad, float4 cells (CQ per voxel, NCELL per thread)
  static constexpr int TS = NCH + 4, CQ = NCH / 4, NCELL = TD * 32 * CQ / THREADS, TB_BYTES = TD * 32 * TS * 4;
  static_assert(THREADS % PARTS == 0, "a thread's slots all carry the same 16-byte part");
};
template <int CG>
using LayoutG = TileLayout<256, 4, CG>;      // k_conv3d_i8<CG>, k_conv3d_i8g<CG>: 4 x 4 x 8 voxels, halo 6 x 6 x 10
using LayoutG2 = TileLayout<256, 2, 16>;     // k_conv3d_i8g2<16>: 2 x 4 x 8, halo 4 x 6 x 10, 64 output channels
using Layout32 = TileLayout<256, 8, 1>;      // k_conv3d_i8l2, k_conv3d_i8l2e: 8 x 4 x 8, halo 10 x 6 x 10, two planes per wave
using LayoutW = TileLayout<512, 4, 2>;       // k_conv3d_i8w: 4 x 4 x 8, 64 output channels
// dynamic LDS of the kernels that keep their tiles there (the kernel carves it, the host asks for it)
template <class L>
constexpr size_t TRANSPOSED_LDS = (size_t)L::HALOB16 + L::TB_BYTES;          // halo tile, transpose buffer
constexpr int W64_WLB = 27 * 2 * 2 * 64 * 16;                               // 110592 bytes of weights
constexpr size_t W64_LDS = (size_t)W64_WLB + LayoutW::HALOB;                // weights, halo tile

struct Lane {
  int tid, li, lh;      // MFMA lane: row / column li, k-half lh
  int plane;            // the wave's (first) d-plane of the tile
  int ch0, chw;         // first output channel of the workgroup / of the wave
};
template <class L>
__device__ __forceinline__ Lane lane_map() {
  Lane ln;
  ln.tid = threadIdx.x;
  const int lane = ln.tid & 63, wid = ln.tid >> 6;
  ln.li = lane & 31;
  ln.lh = lane >> 5;
  ln.plane = wid % L::WPL;
  ln.ch0 = blockIdx.y * L::NCH;
  ln.chw = ln.ch0 + 32 * (wid / L::WPL);
  return ln;
}

// ---- a workgroup's run of tiles, tile index -> first output voxel ---------------------------------------------------------
struct TileRun {
  int begin, end;
};
__device__ __forceinline__ TileRun tile_run(const ConvI8Params& p) {
  const int per = (p.ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
  TileRun r;
  r.begin = (int)blockIdx.x * per;
  r.end = (r.begin + per < p.ntiles) ? r.begin + per : p.ntiles;
  return r;
}
struct Tile {
  int n, od0, oh0, ow0;
};
template <int TD>      // p.tiles_d counts tiles of the kernel's own depth
__device__ __forceinline__ Tile tile_decode(const ConvI8Params& p, int tile) {
  Tile r;
  int t = tile;
  r.ow0 = (t % p.tiles_w) * ITW;
  t /= p.tiles_w;
  r.oh0 = (t % p.tiles_h) * ITH;
  t /= p.tiles_h;
  r.od0 = (t % p.tiles_d) * TD;
  r.n = t / p.tiles_d;
  return r;
}

// ---- epilogue constants ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float epilogue_scale(const ConvI8Params& p) {
  return (float)((double)(*p.act_alpha) * (double)(float)p.wstate->alpha * p.inv_levels);
}
__device__ __forceinline__ float lane_bias(const ConvI8Params& p, const Lane& ln) {
  return (p.bias != nullptr) ? p.bias[ln.chw + ln.li] : 0.0f;
}

// ---- halo slots -----------------------------------------------------------------------------------------------------------
// Slot u = tid + k * THREADS is 16-byte part u % PARTS of halo voxel u / PARTS = (hd, hh, hw); it sits in LDS at
// vox * VS + row * PADB + part * 16 (halo_row_pad).  A thread without a k-th slot gets voxel 0 and lds = -1: its loads
// stay in range and nothing is stored.
struct HaloSlot {
  int hd, hh, hw, lds;
};
template <class L>
__device__ __forceinline__ HaloSlot halo_slot(int tid, int k) {
  const int u = tid + k * L::THREADS;
  const bool live = u < L::NSLOT;
  const int vox = live ? u / L::PARTS : 0;
  HaloSlot s;
  s.hw = vox % I_HW;
  const int row = vox / I_HW;
  s.hh = row % I_HH;
  s.hd = row / I_HH;
  s.lds = live ? vox * L::VS + row * L::PADB + (u % L::PARTS) * 16 : -1;
  return s;
}
template <class L>
__device__ __forceinline__ int halo_part16(int tid) { return (tid % L::PARTS) * 16; }

// per-thread slot constants, independent of the tile: voxel coordinates (clamped loads), LDS offset and global offset
// relative to the tile's first halo voxel (interior loads)
template <class L>
struct HaloTable {
  int cd[L::NHL], ch[L::NHL], cw[L::NHL], lds[L::NHL];
  long long rel[L::NHL];
};
template <class L>
__device__ __forceinline__ void halo_table(const ConvI8Params& p, int tid, HaloTable<L>& t) {
#pragma unroll
  for (int k = 0; k < L::NHL; ++k) {
    const HaloSlot s = halo_slot<L>(tid, k);
    t.cd[k] = s.hd;
    t.ch[k] = s.hh;
    t.cw[k] = s.hw;
    t.lds[k] = s.lds;
    t.rel[k] = (((long long)s.hd * p.H + s.hh) * p.W + s.hw) * L::C1 + halo_part16<L>(tid);
  }
}

// ---- halo prefetch into registers -------------------------------------------------------------------------------------------
// (a) load under the bounds test, zero (level id 0 == zero padding) otherwise
template <class L>
__device__ __forceinline__ void halo_load_tested(const ConvI8Params& p, const Tile& tl, int tid, v4i (&h)[L::NHL]) {
  const int id0 = tl.od0 - p.PD, ih0 = tl.oh0 - p.PH, iw0 = tl.ow0 - p.PW;
#pragma unroll
  for (int k = 0; k < L::NHL; ++k) {
    const HaloSlot s = halo_slot<L>(tid, k);
    const int id = id0 + s.hd, ih = ih0 + s.hh, iw = iw0 + s.hw;
    h[k] = v4i{0, 0, 0, 0};
    if (s.lds >= 0 && id >= 0 && id < p.D && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W)
      h[k] = *reinterpret_cast<const v4i*>(p.x + ((((size_t)tl.n * p.D + id) * p.H + ih) * p.W + iw) * L::C1 +
                                           halo_part16<L>(tid));
  }
}
// (b) unconditional load on clamped coordinates (a load under a branch is waited for in it); the returned validity bits
// are applied when the registers go to LDS
template <class L>
__device__ __forceinline__ unsigned halo_load_clamped(const ConvI8Params& p, const Tile& tl, int tid, const HaloTable<L>& t,
                                                      v4i (&h)[L::NHL]) {
  const int id0 = tl.od0 - p.PD, ih0 = tl.oh0 - p.PH, iw0 = tl.ow0 - p.PW;
  const size_t nbase = (size_t)tl.n * p.D;
  unsigned hm = 0;
#pragma unroll
  for (int k = 0; k < L::NHL; ++k) {
    const int id = id0 + t.cd[k], ih = ih0 + t.ch[k], iw = iw0 + t.cw[k];
    const bool ok = id >= 0 && id < p.D && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
    const int cd = min(max(id, 0), p.D - 1), chh = min(max(ih, 0), p.H - 1), cw = min(max(iw, 0), p.W - 1);
    hm |= (ok ? 1u : 0u) << k;
    h[k] = *reinterpret_cast<const v4i*>(p.x + (((nbase + cd) * p.H + chh) * p.W + cw) * L::C1 + halo_part16<L>(tid));
  }
  return hm;
}
// (c) as (b), but tiles that touch no volume face (uniform over the workgroup) skip clamps and masks: one base per tile
// plus the per-lane offsets of the table; they return all ones
constexpr unsigned HALO_INTERIOR = 0xffffffffu;
template <class L>
__device__ __forceinline__ unsigned halo_load_interior(const ConvI8Params& p, const Tile& tl, int tid, const HaloTable<L>& t,
                                                       v4i (&h)[L::NHL]) {
  const int id0 = tl.od0 - p.PD, ih0 = tl.oh0 - p.PH, iw0 = tl.ow0 - p.PW;
  const bool interior = id0 >= 0 && id0 + L::HD <= p.D && ih0 >= 0 && ih0 + I_HH <= p.H && iw0 >= 0 && iw0 + I_HW <= p.W;
  if (!interior) return halo_load_clamped<L>(p, tl, tid, t, h);
  const int8_t* hb = p.x + ((((long long)tl.n * p.D + id0) * p.H + ih0) * p.W + iw0) * L::C1;
#pragma unroll
  for (int k = 0; k < L::NHL; ++k) h[k] = *reinterpret_cast<const v4i*>(hb + ((t.lds[k] >= 0) ? t.rel[k] : 0));
  return HALO_INTERIOR;
}

// ---- halo registers -> LDS ----------------------------------------------------------------------------------------------
template <class L, bool MASKED>
__device__ __forceinline__ void halo_commit(int8_t* halo, const int (&lds)[L::NHL], const v4i (&h)[L::NHL], unsigned mask) {
#pragma unroll
  for (int k = 0; k < L::NHL; ++k) {
    const v4i val = (!MASKED || ((mask >> k) & 1u)) ? h[k] : v4i{0, 0, 0, 0};   // level id 0 == zero padding
    if (lds[k] >= 0) *reinterpret_cast<v4i*>(&halo[lds[k]]) = val;
  }
}

__device__ __forceinline__ v16i zero_acc() {
  v16i acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0;
  return acc;
}

// ---- tap -> LDS offset of the A fragment: lane -> voxel (h = li >> 3, w = li & 7) of the wave's plane, k-half lh ------------
// The one formula, for halo voxel hv in halo row `row`; the kernels take it split into a lane base and a tap offset
// (ds_read_b128 with the tap as immediate offset), k_conv3d_i8 takes it whole (see there).
template <class L>
__device__ __forceinline__ int a_offset(int hv, int row, int lh, int tap) {
  const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
  return (hv + (kd * I_HH + kh) * I_HW + kw) * L::VS + (row + kd * I_HH + kh) * L::PADB + 16 * lh;
}
__device__ __forceinline__ int lane_halo_row(const Lane& ln) { return ln.plane * I_HH + (ln.li >> 3); }
__device__ __forceinline__ int lane_halo_voxel(const Lane& ln) { return lane_halo_row(ln) * I_HW + (ln.li & 7); }
template <class L>
__device__ __forceinline__ int lane_lds_base(const Lane& ln) {
  return a_offset<L>(lane_halo_voxel(ln), lane_halo_row(ln), ln.lh, 0);
}
template <class L>
__device__ __forceinline__ int tap_lds_offset(int tap) { return a_offset<L>(0, 0, 0, tap); }

// ---- targets and epilogue (a): float4 cells in the transposed layout -------------------------------------------------------
// cell u = tid + k * THREADS is channel quad u % CQ of tile voxel u / CQ
__device__ __forceinline__ bool cell_voxel(const ConvI8Params& p, const Tile& tl, int vox, int& od, int& oh, int& ow) {
  od = tl.od0 + (vox >> 5);
  oh = tl.oh0 + ((vox >> 3) & 3);
  ow = tl.ow0 + (vox & 7);
  return od < p.OD && oh < p.OH && ow < p.OW;
}
// CLAMP: unconditional loads on clamped coordinates, the returned validity bits go to the epilogue; otherwise the load is
// under the bounds test and the epilogue tests again
template <class L, bool CLAMP>
__device__ __forceinline__ unsigned target_load_cells(const ConvI8Params& p, const Tile& tl, const Lane& ln,
                                                      yv4 (&yv)[L::NCELL]) {
  unsigned ym = 0;
#pragma unroll
  for (int k = 0; k < L::NCELL; ++k) {
    const int u = ln.tid + k * L::THREADS;
    int od, oh, ow;
    const bool ok = cell_voxel(p, tl, u / L::CQ, od, oh, ow);
    ym |= (unsigned)ok << k;
    if (CLAMP) {
      od = min(od, p.OD - 1);
      oh = min(oh, p.OH - 1);
      ow = min(ow, p.OW - 1);
    } else {
      yv[k] = yv4{0.f, 0.f, 0.f, 0.f};
    }
    if (CLAMP || ok)
      yv[k] = *reinterpret_cast<const yv4*>(p.y + ((((size_t)tl.n * p.OD + od) * p.OH + oh) * p.OW + ow) * p.C2 + ln.ch0 +
                                            (u % L::CQ) * 4);
  }
  return ym;
}
// scale + bias, transpose through LDS, compare whole 16-byte cells with the prefetched targets: one fp64 add per cell
template <class L, bool MASKED>
__device__ __forceinline__ void epilogue_cells(const ConvI8Params& p, float* tb, const Lane& ln, const v16i& acc, float scale,
                                               float bv, const Tile& tl, const yv4 (&ycur)[L::NCELL], unsigned ymask,
                                               double& l0) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (r & 3) + 8 * (r >> 2) + 4 * ln.lh;
    tb[(ln.plane * 32 + i) * L::TS + (ln.chw - ln.ch0) + ln.li] = (float)acc[r] * scale + bv;
  }
  lds_barrier();
#pragma unroll
  for (int k = 0; k < L::NCELL; ++k) {
    const int u = ln.tid + k * L::THREADS;
    const int vox = u / L::CQ, c4 = u % L::CQ;
    int od, oh, ow;
    const bool ok = MASKED ? (((ymask >> k) & 1u) != 0) : cell_voxel(p, tl, vox, od, oh, ow);
    if (!MASKED && !ok) continue;
    const yv4 o = *reinterpret_cast<const yv4*>(&tb[vox * L::TS + c4 * 4]);
    const float d0 = o[0] - ycur[k][0], d1 = o[1] - ycur[k][1], d2 = o[2] - ycur[k][2], d3 = o[3] - ycur[k][3];
    const double q = ((double)(d0 * d0) + (double)(d1 * d1)) + ((double)(d2 * d2) + (double)(d3 * d3));
    l0 += ok ? q : 0.0;
  }
}

// ---- targets and epilogue in accumulator layout: value r of a lane is voxel (h = r >> 2, w = (r & 3) + 4 lh) of the
// wave's plane(s), channel chw + li - 16 dword loads per lane and plane in 128-byte segments, no LDS transpose ------------
// (b) clamped coordinates plus validity masks; fp64 per value under the mask
template <class L>
__device__ __forceinline__ void target_load_masked(const ConvI8Params& p, const Tile& tl, const Lane& ln,
                                                   float (&y)[L::NPL][16], unsigned (&ymask)[L::NPL]) {
  unsigned rowok = 0, colok = 0;
  size_t rowrel[4];
  int coloff[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int oh = tl.oh0 + q, ow = tl.ow0 + q + 4 * ln.lh;
    rowok |= (unsigned)(oh < p.OH) << q;
    colok |= (unsigned)(ow < p.OW) << q;
    rowrel[q] = (size_t)min(oh, p.OH - 1) * p.OW * p.C2;
    coloff[q] = min(ow, p.OW - 1) * p.C2 + ln.chw + ln.li;
  }
#pragma unroll
  for (int pl = 0; pl < L::NPL; ++pl) {
    const int odr = tl.od0 + ln.plane + 4 * pl;
    const int od = min(odr, p.OD - 1);
    const bool dok = odr < p.OD;
    const size_t ybase = (((size_t)tl.n * p.OD + od) * p.OH) * p.OW * p.C2;
    unsigned ym = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      y[pl][r] = p.y[ybase + rowrel[r >> 2] + coloff[r & 3]];
      ym |= (((rowok >> (r >> 2)) & (colok >> (r & 3)) & 1u) & (dok ? 1u : 0u)) << r;
    }
    ymask[pl] = ym;
  }
}
template <class L>
__device__ __forceinline__ void epilogue_masked(const v16i (&acc)[L::NPL], const float (&ycur)[L::NPL][16],
                                                const unsigned (&ymask)[L::NPL], float scale, float bv, double& l0) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int pl = 0; pl < L::NPL; ++pl) {
      const float d = ((float)acc[pl][r] * scale + bv) - ycur[pl][r];
      l0 += ((ymask[pl] >> r) & 1u) ? (double)(d * d) : 0.0;
    }
}
// (c) the tile divides the volume: targets are always in range, addresses = one base per tile (returned; the output-storing
// epilogue uses it again) + per-lane offsets fixed at start.  Squared errors are accumulated in fp32 within a tile (4
// chains) and added to the fp64 sum once per tile, instead of one fp64 conversion + addition per output value.  OUT: the
// output is also stored, and the attention-weighted sum kept beside the plain one.
__device__ __forceinline__ int acc_voxel_offset(const ConvI8Params& p, const Lane& ln, int r) {
  return ((r >> 2) * p.OW) + (r & 3) + 4 * ln.lh;
}
__device__ __forceinline__ void target_offsets(const ConvI8Params& p, const Lane& ln, int (&yrel)[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) yrel[r] = acc_voxel_offset(p, ln, r) * p.C2 + ln.chw + ln.li;
}
__device__ __forceinline__ long long target_base(const ConvI8Params& p, const Tile& tl, const Lane& ln) {
  return ((((long long)tl.n * p.OD + tl.od0 + ln.plane) * p.OH + tl.oh0) * p.OW + tl.ow0) * p.C2;
}
template <class L>
__device__ __forceinline__ void target_load_even(const ConvI8Params& p, const Tile& tl, const Lane& ln,
                                                 const int (&yrel)[16], float (&y)[L::NPL][16]) {
  const long long yplane = (long long)p.OH * p.OW * p.C2;
  const float* yb = p.y + target_base(p, tl, ln);
#pragma unroll
  for (int r = 0; r < 16; ++r)
#pragma unroll
    for (int pl = 0; pl < L::NPL; ++pl) y[pl][r] = yb[pl * 4 * yplane + yrel[r]];
}
template <class L, bool OUT>
__device__ __forceinline__ void epilogue_even(const ConvI8Params& p, const Lane& ln, const v16i (&acc)[L::NPL],
                                              const float (&ycur)[L::NPL][16], const int (&yrel)[16], long long yoff,
                                              float scale, float bv, double& l0, double& l0w) {
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const long long yplane = (long long)p.OH * p.OW * p.C2, aplane = (long long)p.OH * p.OW;
  float* ob = OUT ? p.out + yoff : nullptr;
  const float* ab = (OUT && p.att != nullptr) ? p.att + yoff / p.C2 : nullptr;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float o[L::NPL], d[L::NPL];
#pragma unroll
    for (int pl = 0; pl < L::NPL; ++pl) o[pl] = (float)acc[pl][r] * scale + bv;
    if (OUT) {
#pragma unroll
      for (int pl = 0; pl < L::NPL; ++pl) ob[pl * 4 * yplane + yrel[r]] = o[pl];
    }
#pragma unroll
    for (int pl = 0; pl < L::NPL; ++pl) d[pl] = o[pl] - ycur[pl][r];
    if (OUT) {
      // (every channel of a voxel adds its weighted error: the sum runs over the values, as the plain one)
      float w[L::NPL];
#pragma unroll
      for (int pl = 0; pl < L::NPL; ++pl) w[pl] = ab ? ab[pl * 4 * aplane + acc_voxel_offset(p, ln, r)] : 1.0f;
#pragma unroll
      for (int pl = 0; pl < L::NPL; ++pl) s[r & 3] = __builtin_fmaf(d[pl], d[pl], s[r & 3]);
#pragma unroll
      for (int pl = 0; pl < L::NPL; ++pl) sw[r & 3] = __builtin_fmaf(w[pl] * d[pl], d[pl], sw[r & 3]);
    } else {
#pragma unroll
      for (int pl = 0; pl < L::NPL; ++pl) s[r & 3] = __builtin_fmaf(d[pl], d[pl], s[r & 3]);
    }
  }
  l0 += (double)((s[0] + s[1]) + (s[2] + s[3]));
  if (OUT) l0w += (double)((sw[0] + sw[1]) + (sw[2] + sw[3]));
}

// ---- the grid-wide sum of the two losses -----------------------------------------------------------------------------------
__device__ __forceinline__ void loss_finish(const ConvI8Params& p, double l0, double l1) {
  __shared__ double red_smem[2 * 16];
  __shared__ int s_last;
  double v[2] = {l0, l1};
  grid_sum_finish<2>(v, p.partials, p.ticket, p.sqerr, red_smem, &s_last, blockIdx.y * gridDim.x + blockIdx.x,
                     gridDim.x * gridDim.y);
}

// ---- tile loop with one register set: the next tile's halo and target cells are prefetched under the current tile's
// MFMAs (forms (a): loads under the bounds test), the epilogue transposes through LDS: k_conv3d_i8g, k_conv3d_i8g2.  mfma()
// is the kernel's own loop over taps and channel groups; it reads A fragments from halo.  (k_conv3d_i8 composes the same
// stages with the clamped forms in a loop of its own, see there.) ------------------------------------------------------
template <class L, class Mfma>
__device__ __forceinline__ void one_set_tiles(const ConvI8Params& p, int8_t* halo, float* tb, const Lane& ln, Mfma mfma) {
  const TileRun run = tile_run(p);
  const float scale = epilogue_scale(p), bv = lane_bias(p, ln);
  double l0 = 0.0;
  v4i hreg[L::NHL];
  yv4 ynext[L::NCELL], ycur[L::NCELL];
#pragma unroll
  for (int k = 0; k < L::NHL; ++k) hreg[k] = v4i{0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < L::NCELL; ++k) ynext[k] = yv4{0.f, 0.f, 0.f, 0.f};
  auto prefetch = [&](int tile) {
    const Tile tl = tile_decode<L::TD>(p, tile);
    halo_load_tested<L>(p, tl, ln.tid, hreg);
    target_load_cells<L, false>(p, tl, ln, ynext);
  };
  if (run.begin < run.end) prefetch(run.begin);
  for (int tile = run.begin; tile < run.end; ++tile) {
    lds_barrier();                                       // halo free (previous tile's MFMAs done)
    int lds[L::NHL];
#pragma unroll
    for (int k = 0; k < L::NHL; ++k) lds[k] = halo_slot<L>(ln.tid, k).lds;
    halo_commit<L, false>(halo, lds, hreg, 0);
#pragma unroll
    for (int k = 0; k < L::NCELL; ++k) ycur[k] = ynext[k];
    lds_barrier();
    if (tile + 1 < run.end) prefetch(tile + 1);
    const v16i acc = mfma();
    epilogue_cells<L, false>(p, tb, ln, acc, scale, bv, tile_decode<L::TD>(p, tile), ycur, 0, l0);
  }
  loss_finish(p, l0, l0);
}

// ---- tile loop with two register sets: the sets alternate roles so that halo and targets are fetched TWO tiles ahead;
// targets and epilogue in accumulator layout.  EVEN: the tile divides the volume - forms (c) of halo prefetch, targets and
// epilogue; otherwise forms (b).  mfma() returns the accumulators of the wave's NPL planes. --------------------------------
template <int NPL>
struct AccSet {
  v16i a[NPL];
};
template <class L>
struct PrefetchRegs {
  v4i h[L::NHL];
  float y[L::NPL][16];
  unsigned hmask, ymask[L::NPL];
};
template <class L>
__device__ __forceinline__ void prefetch_clear(PrefetchRegs<L>& R) {
#pragma unroll
  for (int k = 0; k < L::NHL; ++k) R.h[k] = v4i{0, 0, 0, 0};
#pragma unroll
  for (int pl = 0; pl < L::NPL; ++pl) {
#pragma unroll
    for (int r = 0; r < 16; ++r) R.y[pl][r] = 0.0f;
    R.ymask[pl] = 0;
  }
  R.hmask = 0;
}
template <class L, bool EVEN, bool OUT, class Mfma>
__device__ __forceinline__ void two_set_tiles(const ConvI8Params& p, int8_t* halo, const Lane& ln, Mfma mfma) {
  static_assert(EVEN || !OUT, "only the even-tile epilogue stores the output");
  const TileRun run = tile_run(p);
  const float scale = epilogue_scale(p), bv = lane_bias(p, ln);
  HaloTable<L> ht;
  halo_table<L>(p, ln.tid, ht);
  int yrel[16];
  target_offsets(p, ln, yrel);

  auto fetch = [&](int tile, PrefetchRegs<L>& R) {
    const Tile tl = tile_decode<L::TD>(p, tile);
    if constexpr (EVEN) {
      R.hmask = halo_load_interior<L>(p, tl, ln.tid, ht, R.h);
      target_load_even<L>(p, tl, ln, yrel, R.y);
    } else {
      R.hmask = halo_load_clamped<L>(p, tl, ln.tid, ht, R.h);
      target_load_masked<L>(p, tl, ln, R.y, R.ymask);
    }
  };
  double l0 = 0.0, l0w = 0.0;
  auto body = [&](int tile, PrefetchRegs<L>& X, bool more) {
    lds_barrier();
    if (EVEN && X.hmask == HALO_INTERIOR)
      halo_commit<L, false>(halo, ht.lds, X.h, X.hmask);
    else
      halo_commit<L, true>(halo, ht.lds, X.h, X.hmask);
    float ycur[L::NPL][16];
    unsigned ymask_cur[L::NPL];
#pragma unroll
    for (int pl = 0; pl < L::NPL; ++pl) {
#pragma unroll
      for (int r = 0; r < 16; ++r) ycur[pl][r] = X.y[pl][r];
      ymask_cur[pl] = X.ymask[pl];
    }
    lds_barrier();
    fetch(more ? tile + 2 : tile, X);
    __builtin_amdgcn_sched_barrier(0);
    const AccSet<L::NPL> accs = mfma();
    if constexpr (EVEN)
      epilogue_even<L, OUT>(p, ln, accs.a, ycur, yrel, target_base(p, tile_decode<L::TD>(p, tile), ln), scale, bv, l0, l0w);
    else
      epilogue_masked<L>(accs.a, ycur, ymask_cur, scale, bv, l0);
  };

  // two named sets, passed by reference: an array of sets indexed at run time would go to scratch
  PrefetchRegs<L> A, B;
  prefetch_clear(A);
  prefetch_clear(B);
  if (run.begin < run.end) fetch(run.begin, A);
  if (run.begin + 1 < run.end) fetch(run.begin + 1, B);
  for (int tile = run.begin; tile < run.end; tile += 2) {
    body(tile, A, tile + 2 < run.end);
    if (tile + 1 < run.end) body(tile + 1, B, tile + 3 < run.end);
  }
  loss_finish(p, l0, OUT ? l0w : l0);
}

// ======================================================================================================================
// The kernels
// ======================================================================================================================

// B operands of this wave's 32 output channels in REGISTERS for the whole kernel: lane (j = li, k-half lh) holds 16 channels
// per (tap, group), 27 * CG * 4 VGPRs.  One register set as in one_set_tiles, with the clamped forms of halo prefetch (b) and
// target cells and the sched_barrier behind them.  The loop is written out here and the A addresses come from the whole
// formula, one per tap: through one_set_tiles and a callable, or with a lane base and immediate tap offsets, the scheduler
// no longer issues the LDS reads of a tap's two groups as a pair ahead of their MFMAs (k_conv3d_i8<2>, 16 x 30^3 voxels:
// 0.128 against 0.123 ms).
template <int CG>
__global__ __launch_bounds__(256, (CG == 1) ? 2 : 1) void k_conv3d_i8(ConvI8Params p) {
  using L = LayoutG<CG>;
  constexpr int NHL = L::NHL;
  __shared__ __attribute__((aligned(16))) int8_t halo[L::HALOB];
  __shared__ __attribute__((aligned(16))) float tb[L::TB_BYTES / 4];
  const Lane ln = lane_map<L>();
  const int tid = ln.tid;
  const TileRun run = tile_run(p);
  v4i breg[27][CG];
  {
    const int8_t* wrow = p.wq + ((size_t)(ln.chw + ln.li) * p.C1 + 16 * ln.lh);
#pragma unroll
    for (int tap = 0; tap < 27; ++tap)
#pragma unroll
      for (int g = 0; g < CG; ++g)
        breg[tap][g] = *reinterpret_cast<const v4i*>(wrow + (size_t)tap * p.c2p * p.C1 + 32 * g);
  }
  const float scale = epilogue_scale(p), bv = lane_bias(p, ln);
  HaloTable<L> ht;
  halo_table<L>(p, tid, ht);
  double l0 = 0.0;
  v4i hreg[NHL];
  yv4 ynext[L::NCELL], ycur[L::NCELL];
  unsigned hmask = 0, ymask_next = 0, ymask_cur = 0;
#pragma unroll
  for (int k = 0; k < NHL; ++k) hreg[k] = v4i{0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < L::NCELL; ++k) ynext[k] = yv4{0.f, 0.f, 0.f, 0.f};
  if (run.begin < run.end) {
    const Tile t0 = tile_decode<L::TD>(p, run.begin);
    hmask = halo_load_clamped<L>(p, t0, tid, ht, hreg);
    ymask_next = target_load_cells<L, true>(p, t0, ln, ynext);
  }
  const int hv = lane_halo_voxel(ln), hrow = lane_halo_row(ln);
  for (int tile = run.begin; tile < run.end; ++tile) {
    lds_barrier();                                       // halo free (previous tile's MFMAs done)
    int lds[NHL];
#pragma unroll
    for (int k = 0; k < NHL; ++k) lds[k] = halo_slot<L>(tid, k).lds;
    halo_commit<L, true>(halo, lds, hreg, hmask);
#pragma unroll
    for (int k = 0; k < L::NCELL; ++k) ycur[k] = ynext[k];
    ymask_cur = ymask_next;
    lds_barrier();
    {
      const Tile tn = tile_decode<L::TD>(p, (tile + 1 < run.end) ? tile + 1 : tile);   // the last tile harmlessly re-reads itself
      hmask = halo_load_clamped<L>(p, tn, tid, ht, hreg);
      ymask_next = target_load_cells<L, true>(p, tn, ln, ynext);
    }
    __builtin_amdgcn_sched_barrier(0);
    v16i acc = zero_acc();
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
      const int8_t* arow = halo + a_offset<L>(hv, hrow, ln.lh, tap);
#pragma unroll
      for (int g = 0; g < CG; ++g) {
        const v4i a = *reinterpret_cast<const v4i*>(arow + 32 * g);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, breg[tap][g], acc, 0, 0, 0);
      }
    }
    epilogue_cells<L, true>(p, tb, ln, acc, scale, bv, tile_decode<L::TD>(p, tile), ycur, ymask_cur, l0);
  }
  loss_finish(p, l0, l0);
}

// Wide-channel variant (C1 = 128 / 256): the B operands no longer fit in registers; they stream from L2 through a ring of 8
// registers.  B operand of step (tap, g): wq[((tap*CG + g)*2 + lh) * c2p + chw + li] (16-byte units, k_pack_weight_i8g).
__device__ __forceinline__ const v4i* ring_base(const ConvI8Params& p, const Lane& ln) {
  return reinterpret_cast<const v4i*>(p.wq) + (size_t)ln.lh * p.c2p + ln.chw + ln.li;
}
template <int CG>
__global__ __launch_bounds__(256, (CG <= 4) ? 2 : 1) void k_conv3d_i8g(ConvI8Params p) {
  using L = LayoutG<CG>;
  extern __shared__ __attribute__((aligned(16))) int8_t dyn_lds[];        // TRANSPOSED_LDS<L>
  int8_t* halo = dyn_lds;
  float* tb = reinterpret_cast<float*>(dyn_lds + L::HALOB16);
  const Lane ln = lane_map<L>();
  const v4i* wbase = ring_base(p, ln);
  const size_t wstep = (size_t)2 * p.c2p;
  const int8_t* abase = halo + lane_lds_base<L>(ln);
  one_set_tiles<L>(p, halo, tb, ln, [&]() {
    v16i acc = zero_acc();
    // the ring holds TPA taps: the loads of tap t + TPA are issued right after the MFMAs of tap t (an L2 hit takes ~600
    // cycles, an MFMA 32: one step of look-ahead left the loop latency-bound).  Loads are unconditional on a clamped step
    // index (a load under a branch is waited for in it).
    constexpr int TPA = 8 / CG, NSTEP = 27 * CG;
    v4i bq[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bq[j] = wbase[(size_t)j * wstep];
    auto tap_body = [&](int t, int tj, bool prefetch) {
      const int8_t* arow = abase + tap_lds_offset<L>(t);
#pragma unroll
      for (int g = 0; g < CG; ++g) {
        const v4i a = *reinterpret_cast<const v4i*>(arow + 32 * g);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[tj * CG + g], acc, 0, 0, 0);
        if (prefetch) {
          int nxt = (t + TPA) * CG + g;
          nxt = (nxt < NSTEP) ? nxt : NSTEP - 1;
          bq[tj * CG + g] = wbase[(size_t)nxt * wstep];
        }
      }
    };
    int tap = 0;
#pragma unroll 1
    for (; tap + TPA <= 27 - (27 % TPA == 0 ? TPA : 27 % TPA); tap += TPA) {
#pragma unroll
      for (int tj = 0; tj < TPA; ++tj) tap_body(tap + tj, tj, true);
    }
    // the last group(s): their operands are already in the ring
#pragma unroll 1
    for (; tap + TPA <= 27; tap += TPA) {
#pragma unroll
      for (int tj = 0; tj < TPA; ++tj) tap_body(tap + tj, tj, false);
    }
#pragma unroll
    for (int tj = 0; tj < 27 % TPA; ++tj) tap_body(tap + tj, tj, false);
    return acc;
  });
}

// 512 input channels: the 6 x 6 x 10 halo tile would need 190 KB of LDS, so the tile is 2 x 4 x 8 output voxels (halo
// 4 x 6 x 10 = 127 KB) and the four waves are 2 d-planes x 2 halves of 64 output channels (blockIdx.y counts groups of
// 64).  B operands stream through the same 8-deep register ring, one ring load per MFMA step (tap, group).
template <int CG>
__global__ __launch_bounds__(256, 1) void k_conv3d_i8g2(ConvI8Params p) {
  static_assert(CG % 8 == 0, "ring blocks of 8 steps must not straddle taps");
  using L = TileLayout<256, 2, CG>;
  extern __shared__ __attribute__((aligned(16))) int8_t dyn_lds[];        // TRANSPOSED_LDS<L>
  int8_t* halo = dyn_lds;
  float* tb = reinterpret_cast<float*>(dyn_lds + L::HALOB16);
  const Lane ln = lane_map<L>();
  const v4i* wbase = ring_base(p, ln);
  const size_t wstep = (size_t)2 * p.c2p;
  const int8_t* abase = halo + lane_lds_base<L>(ln);
  one_set_tiles<L>(p, halo, tb, ln, [&]() {
    v16i acc = zero_acc();
    constexpr int NSTEP = 27 * CG;
    v4i bq[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bq[j] = wbase[(size_t)j * wstep];
#pragma unroll 1
    for (int s0 = 0; s0 < NSTEP; s0 += 8) {
      const int t = s0 / CG, g0 = s0 % CG;                  // 8 | CG: the tap is constant inside a block of 8 steps
      const int8_t* arow = abase + tap_lds_offset<L>(t) + 32 * g0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const v4i a = *reinterpret_cast<const v4i*>(arow + 32 * j);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[j], acc, 0, 0, 0);
        int nxt = s0 + 8 + j;
        nxt = (nxt < NSTEP) ? nxt : NSTEP - 1;              // unconditional load on a clamped index
        bq[j] = wbase[(size_t)nxt * wstep];
      }
      // keeps the ring loads in the iteration that issues them: without it the optimiser may merge them with the loads
      // before the loop into loads at the top of the NEXT iteration, which wait in it (no look-ahead, +13 %)
      asm volatile("" ::: "memory");
    }
    return acc;
  });
}

// 32-input-channel kernels, tuned for memory-level parallelism (they are HBM-latency bound): B operands (27 KB) live in LDS,
// laid out [tap][k-half][out channel][16 B] (conflict-free ds_read_b128); two register sets alternate roles so that halo
// and targets are fetched TWO tiles ahead; targets are fetched in accumulator layout, so the epilogue needs no LDS
// transpose.  A workgroup tile is 8x4x8 output voxels, wave w owns d-planes w and w+4 and feeds BOTH accumulators from one
// read of the B operand (a one-plane tile was bound by its LDS operand traffic, 27 x 2 KB per wave-tile); barriers, tile
// decoding and halo overlap are amortised over twice the voxels.  2 workgroups per CU.
template <bool EVEN, bool OUT>
__device__ __forceinline__ void conv3d_i8_c32(const ConvI8Params& p) {
  using L = Layout32;
  __shared__ __attribute__((aligned(16))) int8_t wl[27 * 2 * 32 * 16];
  __shared__ __attribute__((aligned(16))) int8_t halo[L::HALOB];
  const Lane ln = lane_map<L>();
  for (int u = ln.tid; u < 27 * 2 * 32; u += 256) {
    const int j = u & 31, h = (u >> 5) & 1, tap = u >> 6;
    *reinterpret_cast<v4i*>(&wl[u * 16]) =
        *reinterpret_cast<const v4i*>(p.wq + ((size_t)(tap * p.c2p + ln.ch0 + j) * 32 + 16 * h));
  }
  if (EVEN) lds_barrier();      // (otherwise the first barrier of the tile loop covers wl)
  const int hb0 = lane_lds_base<L>(ln), hb1 = hb0 + 4 * I_HH * L::ROWB;
  two_set_tiles<L, EVEN, OUT>(p, halo, ln, [&]() {
    v16i acc0 = zero_acc(), acc1 = zero_acc();
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
      const int toff = tap_lds_offset<L>(tap);
      const v4i b = *reinterpret_cast<const v4i*>(&wl[((tap * 2 + ln.lh) * 32 + ln.li) * 16]);
      const v4i a0 = *reinterpret_cast<const v4i*>(halo + hb0 + toff);
      const v4i a1 = *reinterpret_cast<const v4i*>(halo + hb1 + toff);
      acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b, acc1, 0, 0, 0);
    }
    return AccSet<2>{{acc0, acc1}};
  });
}
// This variant takes ragged volumes and any C2 % 32 == 0; k_conv3d_i8l2e is its fast path.
__global__ __launch_bounds__(256, 2) void k_conv3d_i8l2(ConvI8Params p) { conv3d_i8_c32<false, false>(p); }

// ---- k_conv3d_i8l2 for volumes the 8 x 4 x 8 tile divides (every shape of the shipped recipes), 32 -> 32 channels -----------
// Same tiling and arithmetic as k_conv3d_i8l2, with the per-tile VALU work cut from ~790 to ~300 instructions per wave
// (PMC: 54 MFMAs against 787 VALU instructions per wave-tile made the kernel VALU-issue bound, profiles/r02_pmc_i8l2):
// forms (c) of the halo prefetch, the target prefetch and the epilogue.
//
// The output-storing form keeps a copy of its own, stages written out: it needs more than 256 registers (324 bytes of
// scratch per lane) and what it spills decides its speed - composed of the shared stages it spilled less (268 - 308 bytes)
// and ran 6 - 14 % slower (0.539 - 0.582 against 0.510 ms per conv_forward_i8 at 16 x 64^3, profiles/conv_i8_shared_ab.txt).
template <bool OUT>
__global__ __launch_bounds__(256, 2) void k_conv3d_i8l2e(ConvI8Params p) {
  if constexpr (!OUT) {
    conv3d_i8_c32<true, false>(p);
    return;
  }
  using L = Layout32;
  constexpr int VS = L::VS, PADB = L::PADB, NHL = L::NHL, L2_NH = L::NVOX, L2_HD = L::HD, L2_TD = L::TD;
  __shared__ __attribute__((aligned(16))) int8_t wl[27 * 2 * 32 * 16];
  __shared__ __attribute__((aligned(16))) int8_t halo[L::HALOB];
  __shared__ double red_smem[2 * 16];
  __shared__ int s_last;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int per = (p.ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
  const int t_begin = (int)blockIdx.x * per;
  const int t_end = (t_begin + per < p.ntiles) ? t_begin + per : p.ntiles;

  for (int u = tid; u < 27 * 2 * 32; u += 256) {
    const int j = u & 31, h = (u >> 5) & 1, tap = u >> 6;
    *reinterpret_cast<v4i*>(&wl[u * 16]) = *reinterpret_cast<const v4i*>(p.wq + ((size_t)(tap * p.c2p + j) * 32 + 16 * h));
  }
  lds_barrier();
  const float scale = (float)((double)(*p.act_alpha) * (double)(float)p.wstate->alpha * p.inv_levels);
  const float bv = (p.bias != nullptr) ? p.bias[li] : 0.0f;

  // per-lane constants: halo voxel of each of the 5 loads (relative coordinates, LDS offset, global offset relative to
  // the tile's first halo voxel), target offsets of the 2 x 16 outputs relative to the tile's first output voxel
  int hcd[NHL], hch[NHL], hcw[NHL], hlds[NHL];
  long long hrel[NHL];
#pragma unroll
  for (int k = 0; k < NHL; ++k) {
    const int u = tid + k * 256;
    const int vox = (u < L2_NH * 2) ? (u >> 1) : 0;
    hcw[k] = vox % I_HW;
    const int t2 = vox / I_HW;
    hch[k] = t2 % I_HH;
    hcd[k] = t2 / I_HH;
    hlds[k] = (u < L2_NH * 2) ? vox * VS + t2 * PADB + (u & 1) * 16 : -1;
    hrel[k] = (((long long)hcd[k] * p.H + hch[k]) * p.W + hcw[k]) * 32 + (tid & 1) * 16;
  }
  int yrel[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) yrel[r] = (((r >> 2) * p.OW) + (r & 3) + 4 * lh) * p.C2 + li;
  const long long yplane = (long long)p.OH * p.OW * p.C2;

  struct Regs {
    v4i h[NHL];
    float y[2][16];
    unsigned hmask;
    long long yoff;      // (OUT) the tile's first output value of this wave's plane, relative to p.y
  };
  auto fetch = [&](int tile, Regs& R) {
    const Tile tl = tile_decode<L2_TD>(p, tile);
    const int n = tl.n, od0 = tl.od0, oh0 = tl.oh0, ow0 = tl.ow0;
    const int id0 = od0 - p.PD, ih0 = oh0 - p.PH, iw0 = ow0 - p.PW;
    const bool interior = id0 >= 0 && id0 + L2_HD <= p.D && ih0 >= 0 && ih0 + I_HH <= p.H && iw0 >= 0 && iw0 + I_HW <= p.W;
    if (interior) {                       // uniform over the workgroup
      const int8_t* hb = p.x + ((((long long)n * p.D + id0) * p.H + ih0) * p.W + iw0) * 32;
#pragma unroll
      for (int k = 0; k < NHL; ++k) R.h[k] = *reinterpret_cast<const v4i*>(hb + ((hlds[k] >= 0) ? hrel[k] : 0));
      R.hmask = 0xffffffffu;
    } else {
      const size_t nbase = (size_t)n * p.D;
      unsigned hm = 0;
#pragma unroll
      for (int k = 0; k < NHL; ++k) {
        const int id = id0 + hcd[k], ih = ih0 + hch[k], iw = iw0 + hcw[k];
        const bool ok = id >= 0 && id < p.D && ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
        const int cd = min(max(id, 0), p.D - 1), chh = min(max(ih, 0), p.H - 1), cw = min(max(iw, 0), p.W - 1);
        hm |= (ok ? 1u : 0u) << k;
        R.h[k] = *reinterpret_cast<const v4i*>(p.x + (((nbase + cd) * p.H + chh) * p.W + cw) * 32 + (tid & 1) * 16);
      }
      R.hmask = hm;
    }
    const long long yoff = ((((long long)n * p.OD + od0 + wid) * p.OH + oh0) * p.OW + ow0) * p.C2;
    const float* yb = p.y + yoff;
    R.yoff = yoff;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      R.y[0][r] = yb[yrel[r]];
      R.y[1][r] = yb[4 * yplane + yrel[r]];
    }
  };

  const int hv0 = (wid * I_HH + (li >> 3)) * I_HW + (li & 7);
  const int hb0 = hv0 * VS + (wid * I_HH + (li >> 3)) * PADB + 16 * lh;
  const int hb1 = hb0 + 4 * I_HH * (I_HW * VS + PADB);
  double l0 = 0.0, l0w = 0.0;
  auto body = [&](int tile, Regs& X, bool more) {
    const long long yoff_cur = X.yoff;
    lds_barrier();
    if (X.hmask == 0xffffffffu) {
#pragma unroll
      for (int k = 0; k < NHL; ++k)
        if (hlds[k] >= 0) *reinterpret_cast<v4i*>(&halo[hlds[k]]) = X.h[k];
    } else {
#pragma unroll
      for (int k = 0; k < NHL; ++k) {
        const v4i val = ((X.hmask >> k) & 1u) ? X.h[k] : v4i{0, 0, 0, 0};
        if (hlds[k] >= 0) *reinterpret_cast<v4i*>(&halo[hlds[k]]) = val;
      }
    }
    float ycur[2][16];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
      for (int r = 0; r < 16; ++r) ycur[pl][r] = X.y[pl][r];
    lds_barrier();
    fetch(more ? tile + 2 : tile, X);
    __builtin_amdgcn_sched_barrier(0);
    v16i acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0;
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
      const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
      const int toff = ((kd * I_HH + kh) * I_HW + kw) * VS + (kd * I_HH + kh) * PADB;
      const v4i b = *reinterpret_cast<const v4i*>(&wl[((tap * 2 + lh) * 32 + li) * 16]);
      const v4i a0 = *reinterpret_cast<const v4i*>(halo + hb0 + toff);
      const v4i a1 = *reinterpret_cast<const v4i*>(halo + hb1 + toff);
      acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b, acc1, 0, 0, 0);
    }
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (OUT) {
      float sw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      float* ob = p.out + yoff_cur;
      const float* ab = (p.att != nullptr) ? p.att + yoff_cur / p.C2 : nullptr;
      const long long aplane = (long long)p.OH * p.OW;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int arel = ((r >> 2) * p.OW) + (r & 3) + 4 * lh;
        const float o0 = (float)acc0[r] * scale + bv, o1 = (float)acc1[r] * scale + bv;
        ob[yrel[r]] = o0;
        ob[4 * yplane + yrel[r]] = o1;
        const float d0 = o0 - ycur[0][r], d1 = o1 - ycur[1][r];
        const float w0 = ab ? ab[arel] : 1.0f, w1 = ab ? ab[4 * aplane + arel] : 1.0f;
        s[r & 3] = __builtin_fmaf(d0, d0, s[r & 3]);
        s[r & 3] = __builtin_fmaf(d1, d1, s[r & 3]);
        sw[r & 3] = __builtin_fmaf(w0 * d0, d0, sw[r & 3]);
        sw[r & 3] = __builtin_fmaf(w1 * d1, d1, sw[r & 3]);
      }
      l0w += (double)((sw[0] + sw[1]) + (sw[2] + sw[3]));
    }
    l0 += (double)((s[0] + s[1]) + (s[2] + s[3]));
  };

  Regs A, B;
#pragma unroll
  for (int k = 0; k < NHL; ++k) A.h[k] = B.h[k] = v4i{0, 0, 0, 0};
#pragma unroll
  for (int pl = 0; pl < 2; ++pl)
#pragma unroll
    for (int r = 0; r < 16; ++r) A.y[pl][r] = B.y[pl][r] = 0.0f;
  A.hmask = B.hmask = 0;
  A.yoff = B.yoff = 0;
  if (t_begin < t_end) fetch(t_begin, A);
  if (t_begin + 1 < t_end) fetch(t_begin + 1, B);
  for (int tile = t_begin; tile < t_end; tile += 2) {
    body(tile, A, tile + 2 < t_end);
    if (tile + 1 < t_end) body(tile + 1, B, tile + 3 < t_end);
  }
  double v[2] = {l0, l0w};
  grid_sum_finish<2>(v, p.partials, p.ticket, p.sqerr, red_smem, &s_last, blockIdx.y * gridDim.x + blockIdx.x,
                     gridDim.x * gridDim.y);
}

// ---- 64 -> 64 channels with the weights in LDS ------------------------------------------------------------------------
// k_conv3d_i8<2> keeps the 54 B operands of a wave in 216 registers: one workgroup of 4 waves per CU, nothing to hide the
// halo staging, the barriers and the transposed epilogue behind (0.122 ms for 16 x 32^3 voxels: 17 % of the HBM stream,
// 5x its MFMA time).  Here ALL weights (64 x 64 x 27 bytes = 108 KB, packed [tap][group][k half][out channel][16 B]) sit in
// LDS beside the 6 x 6 x 10 halo tile (31.5 KB): one workgroup of 8 waves per CU - wave w owns d-plane w & 3 and output
// channels 32 (w >> 2) .. +31 of a 4 x 4 x 8 tile - with ~100 registers per wave and the tile loop of k_conv3d_i8l2e.
// Tile-divisible volumes only (every shape of the shipped recipes); other shapes keep k_conv3d_i8<2>.
template <bool OUT>
__global__ __launch_bounds__(512, 1) void k_conv3d_i8w(ConvI8Params p) {
  using L = LayoutW;
  extern __shared__ __attribute__((aligned(16))) int8_t dyn_lds[];        // W64_LDS
  int8_t* wl = dyn_lds;
  int8_t* halo = dyn_lds + W64_WLB;
  const Lane ln = lane_map<L>();
  for (int u = ln.tid; u < W64_WLB / 16; u += 512)
    reinterpret_cast<v4i*>(wl)[u] = reinterpret_cast<const v4i*>(p.wq)[u];
  lds_barrier();
  const int hb0 = lane_lds_base<L>(ln);
  const int8_t* wlane = wl + ((size_t)ln.lh * 64 + ln.chw + ln.li) * 16;        // + (tap * 2 + g) * 2 * 64 * 16 per step
  two_set_tiles<L, true, OUT>(p, halo, ln, [&]() {
    v16i acc0 = zero_acc(), acc1 = zero_acc();                       // one chain per channel group
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
      const int toff = tap_lds_offset<L>(tap);
      const v4i a0 = *reinterpret_cast<const v4i*>(halo + hb0 + toff);
      const v4i a1 = *reinterpret_cast<const v4i*>(halo + hb0 + toff + 32);
      const v4i b0 = *reinterpret_cast<const v4i*>(wlane + (size_t)(tap * 2 + 0) * 2 * 64 * 16);
      const v4i b1 = *reinterpret_cast<const v4i*>(wlane + (size_t)(tap * 2 + 1) * 2 * 64 * 16);
      acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc1, 0, 0, 0);
    }
    return AccSet<1>{{acc0 + acc1}};       // exact: the integer sum before the one scale
  });
}

struct I8Plan {
  ConvI8Params p;
  dim3 grid;
  size_t nblk, wq_bytes;
};

// The ids effq_conv_i8_plan_query reports (effq_hip.h, hip_ops.CONV_I8_KERNELS)
enum I8Kernel {
  I8K_NONE = 0,     // an output is wanted and no output-storing kernel serves the shape
  I8K_L2E = 1,      // k_conv3d_i8l2e
  I8K_L2 = 2,       // k_conv3d_i8l2
  I8K_R64 = 3,      // k_conv3d_i8<2>
  I8K_W = 4,        // k_conv3d_i8w
  I8K_G4 = 5,       // k_conv3d_i8g<4>
  I8K_G8 = 6,       // k_conv3d_i8g<8>
  I8K_G2 = 7        // k_conv3d_i8g2<16>
};

// the kernel, stride and channel counts some kernel of this file serves
static bool i8_geom_ok(const effq_geom* g) {
  if (!(g->KD == 3 && g->KH == 3 && g->KW == 3 && g->SD == 1 && g->SH == 1 && g->SW == 1)) return false;
  if (!(g->C1 == 32 || g->C1 == 64 || g->C1 == 128 || g->C1 == 256 || g->C1 == 512)) return false;
  return g->C2 > 0 && (g->C2 % 32) == 0 && (g->C1 != 512 || (g->C2 % 64) == 0);
}

static int i8_plan(const effq_geom* g, I8Plan* pl) {
  EFFQ_CHECK_ARG(g != nullptr);
  EFFQ_CHECK_ARG(i8_geom_ok(g));
  EFFQ_CHECK_ARG(g->N > 0 && g->D > 0 && g->H > 0 && g->W > 0 && g->PD >= 0 && g->PH >= 0 && g->PW >= 0);
  ConvI8Params& p = pl->p;
  memset(&p, 0, sizeof(p));
  p.N = g->N; p.C1 = g->C1; p.C2 = g->C2; p.c2p = g->C2; p.D = g->D; p.H = g->H; p.W = g->W;
  p.PD = g->PD; p.PH = g->PH; p.PW = g->PW;
  p.OD = g->D + 2 * g->PD - 2; p.OH = g->H + 2 * g->PH - 2; p.OW = g->W + 2 * g->PW - 2;
  EFFQ_CHECK_ARG(p.OD > 0 && p.OH > 0 && p.OW > 0);
  const int td = (g->C1 == 32) ? Layout32::TD : (g->C1 == 512) ? LayoutG2::TD : LayoutG<2>::TD;
  static_assert(LayoutW::TD == LayoutG<2>::TD, "64 -> 64: one plan serves k_conv3d_i8w and k_conv3d_i8<2>");
  p.tiles_d = (p.OD + td - 1) / td;
  p.tiles_h = (p.OH + ITH - 1) / ITH;
  p.tiles_w = (p.OW + ITW - 1) / ITW;
  const long long nt = (long long)p.N * p.tiles_d * p.tiles_h * p.tiles_w;
  EFFQ_CHECK_ARG(nt < (1ll << 30));
  p.ntiles = (int)nt;
  const int ny = (g->C1 == 512) ? p.C2 / 64 : p.C2 / 32;
  const int wg_per_cu = (g->C1 == 32 || g->C1 == 128) ? 2 : 1;
  int gx = (256 * wg_per_cu + ny - 1) / ny;
  if (gx < 32) gx = 32;
  // The persistent grid leaves a few workgroup slots empty: the chain kernels of the NEXT iterate (prox GEMM, scale fixed
  // point, projection) run beside this kernel and otherwise find no room until the persistent workgroups retire - chain
  // and loss then serialise (32-channel layers: 0.104 ms per prox solve in situ against 0.046 with 15 slots free (grid 497; 482 workgroups measured worse again),
  // 1222 -> 1190 ms per calibration).  The grid is trimmed to equal runs of tiles.
  constexpr int rsv = 15;
  if (gx * ny > 2 * rsv) {
    int g0 = gx - (rsv + ny - 1) / ny;
    const int per = (p.ntiles + g0 - 1) / g0;
    gx = (p.ntiles + per - 1) / per;
  }
  if (gx > p.ntiles) gx = p.ntiles;
  pl->grid = dim3((unsigned)gx, (unsigned)ny, 1);
  pl->nblk = (size_t)gx * ny;
  if (pl->nblk < 256) pl->nblk = 256;      // k_conv3d_i8w runs one workgroup per CU whatever the plan above says
  pl->wq_bytes = (size_t)27 * p.c2p * p.C1;
  return EFFQ_OK;
}

// workspace: the ticket (256 bytes), two partial sums per workgroup, the packed weights and the slack to align them
static size_t i8_ws_bytes(const I8Plan& pl) { return 256 + pl.nblk * 2 * sizeof(double) + pl.wq_bytes + 256; }

// 32 -> 32 layers whose output tiles evenly: k_conv3d_i8l2e
static bool i8_l2e(const ConvI8Params& p) {
  return p.C1 == 32 && p.C2 == 32 && p.OD % Layout32::TD == 0 && p.OH % ITH == 0 && p.OW % ITW == 0;
}
// 64 -> 64 layers whose output tiles evenly: k_conv3d_i8w
static bool i8_w64(const ConvI8Params& p) {
  return p.C1 == 64 && p.C2 == 64 && p.OD % LayoutW::TD == 0 && p.OH % ITH == 0 && p.OW % ITW == 0;
}
// the shapes whose kernel can also store its output
static bool i8_has_out(const ConvI8Params& p) { return i8_l2e(p) || i8_w64(p); }

// The kernel conv_i8_impl launches and its grid.x (effq_conv_i8_plan_query reports both)
static I8Kernel i8_kernel(const I8Plan& pl, bool want_out, int* grid_x) {
  const ConvI8Params& p = pl.p;
  *grid_x = (int)pl.grid.x;
  if (want_out && !i8_has_out(p)) return I8K_NONE;
  if (i8_w64(p)) {
    int gx = 256;                           // one workgroup per CU (LDS); pl.nblk = 256 partial slots
    if (gx > p.ntiles) gx = p.ntiles;
    if ((size_t)gx > pl.nblk) gx = (int)pl.nblk;
    *grid_x = gx;
    return I8K_W;
  }
  if (p.C1 == 32) return i8_l2e(p) ? I8K_L2E : I8K_L2;
  if (p.C1 == 64) return I8K_R64;
  return p.C1 == 512 ? I8K_G2 : p.C1 == 128 ? I8K_G4 : I8K_G8;
}

}  // namespace effq

using namespace effq;

extern "C" {

int effq_conv_i8_supported(const effq_geom* g, int act_levels, int w_levels) {
  if (g == nullptr || !i8_geom_ok(g)) return 0;
  if (act_levels < 2 || act_levels > 128 || w_levels < 2 || w_levels > 128) return 0;
  // int32 accumulator range: 27*C1 products of at most (La-1)*(Lw-1)
  if ((double)27 * g->C1 * (act_levels - 1) * (w_levels - 1) >= 2147483647.0) return 0;
  return 1;
}

size_t effq_conv_i8_ws_bytes(const effq_geom* g) {
  I8Plan pl;
  if (i8_plan(g, &pl) != EFFQ_OK) return 0;
  return i8_ws_bytes(pl);
}

int effq_conv_i8_out_supported(const effq_geom* g, int act_levels, int w_levels) {
  if (g == nullptr || !effq_conv_i8_supported(g, act_levels, w_levels)) return 0;
  I8Plan pl;
  if (i8_plan(g, &pl) != EFFQ_OK) return 0;
  return i8_has_out(pl.p) ? 1 : 0;
}

static int conv_i8_impl(const uint8_t* xidx_ndhwc, const int8_t* Gq, const float* bias, const float* y_fp,
                        const effq_geom* g, const float* act_alpha_dev, int act_levels,
                        const effq_fp_state* w_state_dev, int w_levels, double* sqerr_out, void* ws, size_t ws_bytes,
                        void* stream, float* out, const float* att) {
  EFFQ_CHECK_ARG(xidx_ndhwc && Gq && y_fp && g && act_alpha_dev && w_state_dev && sqerr_out && ws);
  EFFQ_CHECK_ARG(effq_conv_i8_supported(g, act_levels, w_levels));
  I8Plan pl;
  int rc = i8_plan(g, &pl);
  if (rc != EFFQ_OK) return rc;
  const size_t need = i8_ws_bytes(pl);
  if (ws_bytes < need) {
    set_error("conv_i8: workspace %zu < required %zu", ws_bytes, need);
    return EFFQ_ERR_WORKSPACE;
  }
  char* base = reinterpret_cast<char*>(ws);
  ConvI8Params& p = pl.p;
  p.ticket = reinterpret_cast<unsigned int*>(base);
  p.partials = reinterpret_cast<double*>(base + 256);
  int8_t* wq = reinterpret_cast<int8_t*>(base + 256 + pl.nblk * 2 * sizeof(double));
  wq = reinterpret_cast<int8_t*>((reinterpret_cast<uintptr_t>(wq) + 15) & ~(uintptr_t)15);
  p.x = reinterpret_cast<const int8_t*>(xidx_ndhwc);
  p.wq = wq;
  p.bias = bias;
  p.y = y_fp;
  p.act_alpha = act_alpha_dev;
  p.wstate = w_state_dev;
  p.inv_levels = 1.0 / ((double)(act_levels - 1) * (double)(w_levels - 1));
  p.sqerr = sqerr_out;
  p.out = out;
  p.att = att;
  int gx = 0;
  const I8Kernel kern = i8_kernel(pl, out != nullptr, &gx);
  if (kern == I8K_NONE) {
    set_error("conv_i8: no output-storing kernel for this shape (effq_conv_i8_out_supported)");
    return EFFQ_ERR_ARG;
  }
  hipStream_t st = as_stream(stream);
  // (the ticket of the last-block reduction is left at zero by the kernel that used it: the caller zero-fills
  //  the workspace once, effq_hip.h)
  if (kern == I8K_W) {
    hipLaunchKernelGGL(k_pack_weight_i8g<4>, dim3((unsigned)((p.c2p + 3) / 4)), dim3(256), (size_t)4 * p.C1 * 27, st, Gq, wq, p.C1, p.C2, 27, p.c2p);
    EFFQ_HIP(raise_lds_limit<k_conv3d_i8w<false>>(W64_LDS));
    EFFQ_HIP(raise_lds_limit<k_conv3d_i8w<true>>(W64_LDS));
    if (out != nullptr)
      hipLaunchKernelGGL(k_conv3d_i8w<true>, dim3((unsigned)gx), dim3(512), W64_LDS, st, p);
    else
      hipLaunchKernelGGL(k_conv3d_i8w<false>, dim3((unsigned)gx), dim3(512), W64_LDS, st, p);
    EFFQ_LAUNCH_CHECK();
    return EFFQ_OK;
  }
  {
    size_t nb = (pl.wq_bytes + 255) / 256;
    if (nb > 2048) nb = 2048;
    if (p.C1 <= 64)
      hipLaunchKernelGGL(k_pack_weight_i8, dim3((unsigned)nb), dim3(256), 0, st, Gq, wq, p.C1, p.C2, 27, p.c2p);
    else   // the pack sits on the loss stream beside the ADMM chain: one output channel per workgroup (128 - 512
           // workgroups instead of 32 - 128 with four channels each) shortens it
      hipLaunchKernelGGL(k_pack_weight_i8g<1>, dim3((unsigned)p.c2p), dim3(256), (size_t)p.C1 * 27, st, Gq, wq, p.C1, p.C2, 27, p.c2p);
    EFFQ_LAUNCH_CHECK();
  }
  switch (kern) {
    case I8K_L2E:
      if (out != nullptr)
        hipLaunchKernelGGL(k_conv3d_i8l2e<true>, pl.grid, dim3(256), 0, st, p);
      else
        hipLaunchKernelGGL(k_conv3d_i8l2e<false>, pl.grid, dim3(256), 0, st, p);
      break;
    case I8K_L2:
      hipLaunchKernelGGL(k_conv3d_i8l2, pl.grid, dim3(256), 0, st, p);
      break;
    case I8K_R64:
      hipLaunchKernelGGL(k_conv3d_i8<2>, pl.grid, dim3(256), 0, st, p);
      break;
    case I8K_G4:
      EFFQ_HIP(raise_lds_limit<k_conv3d_i8g<4>>(TRANSPOSED_LDS<LayoutG<4>>));
      hipLaunchKernelGGL(k_conv3d_i8g<4>, pl.grid, dim3(256), TRANSPOSED_LDS<LayoutG<4>>, st, p);
      break;
    case I8K_G8:
      EFFQ_HIP(raise_lds_limit<k_conv3d_i8g<8>>(TRANSPOSED_LDS<LayoutG<8>>));
      hipLaunchKernelGGL(k_conv3d_i8g<8>, pl.grid, dim3(256), TRANSPOSED_LDS<LayoutG<8>>, st, p);
      break;
    default:      // I8K_G2
      EFFQ_HIP(raise_lds_limit<k_conv3d_i8g2<16>>(TRANSPOSED_LDS<LayoutG2>));
      hipLaunchKernelGGL(k_conv3d_i8g2<16>, pl.grid, dim3(256), TRANSPOSED_LDS<LayoutG2>, st, p);
      break;
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// the launch conv3d_calib_step_i8 (want_out == 0) or conv3d_quant_forward_i8 makes for a geometry (launches nothing): the
// same i8_plan and i8_kernel
int effq_conv_i8_plan_query(const effq_geom* g, int want_out, int* kernel, int* grid_x, int* grid_y, int* ntiles) {
  EFFQ_CHECK_ARG(kernel && grid_x && grid_y && ntiles);
  I8Plan pl;
  const int rc = i8_plan(g, &pl);
  if (rc != EFFQ_OK) return rc;
  *kernel = i8_kernel(pl, want_out != 0, grid_x);
  if (*kernel == I8K_NONE) {
    set_error("conv_i8: no output-storing kernel for this shape (effq_conv_i8_out_supported)");
    return EFFQ_ERR_ARG;
  }
  *grid_y = (*kernel == I8K_W) ? 1 : (int)pl.grid.y;
  *ntiles = pl.p.ntiles;
  return EFFQ_OK;
}

int conv3d_calib_step_i8(const uint8_t* xidx_ndhwc, const int8_t* Gq, const float* bias, const float* y_fp,
                         const effq_geom* g, const float* act_alpha_dev, int act_levels,
                         const effq_fp_state* w_state_dev, int w_levels, double* sqerr_out, void* ws, size_t ws_bytes,
                         void* stream) {
  return conv_i8_impl(xidx_ndhwc, Gq, bias, y_fp, g, act_alpha_dev, act_levels, w_state_dev, w_levels, sqerr_out, ws,
                      ws_bytes, stream, nullptr, nullptr);
}

int conv3d_quant_forward_i8(const uint8_t* xidx_ndhwc, const int8_t* Gq, const float* bias, const float* y_fp,
                            const float* att, const effq_geom* g, const float* act_alpha_dev, int act_levels,
                            const effq_fp_state* w_state_dev, int w_levels, double* sqerr_out, float* out, void* ws,
                            size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(out != nullptr);
  return conv_i8_impl(xidx_ndhwc, Gq, bias, y_fp, g, act_alpha_dev, act_levels, w_state_dev, w_levels, sqerr_out, ws,
                      ws_bytes, stream, out, att);
}

}  // extern "C"
