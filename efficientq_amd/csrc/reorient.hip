// Reorientation of the `prep` and `predict` missions (prep.py, --prep_orient): N volumes x (N, D, H, W) of 4-byte or 1-byte
// elements become y (N, dims[src_axis[0]], dims[src_axis[1]], dims[src_axis[2]]): output axis p is source axis src_axis[p],
// reversed iff bit p of flip_mask is set.  A permutation of the voxels: values are moved as 32-bit words or bytes and never
// interpreted (a NaN keeps its payload), there is no atomic and no reduction, equal inputs give equal bits.
//
// Variant 0 (src_axis[2] == 2, source W stays innermost): k_reorient_rows.  A thread moves 16 consecutive bytes of one
//   output row (4 floats or 16 bytes) with one 16-B load and one 16-B store; a reversed row is read from its mirrored place
//   and reversed inside the vector; the last W % 4 (W % 16) elements of a row go one by one.
// Variant 1 (the innermost output axis is source D or H, call it `a`; `b` is the other of the two): a tiled transpose
//   through LDS over the plane of source W and a; b and N are walked by the (flattened) grid.  Global reads run along
//   source W, global writes along output W (= a); the flips are applied to the destination coordinates of the tile.
//   fp32, k_reorient_tile_f32: tiles of 64 x 64 words in LDS rows of 65 words.  A wave writes tile[r][lane] (bank
//     (65 r + lane) % 32 = (r + lane) % 32: the 32 lanes of a half differ) and reads tile[lane][r] (bank (65 lane + r)
//     % 32 = (lane + r) % 32: likewise), so neither side has a bank conflict; both global sides are 256 B per wave.
//   uint8, k_reorient_tile_u8: tiles of 128 (a) x 128 (W) bytes, kept as 128 rows of 32 words as they were loaded, word c
//     of row r at column (c + r / 4) % 32.  A half-wave writes the 32 words of one row (columns all different) and, in the
//     second phase, lane j of a half reads word c of the rows 4 j ... 4 j + 3 (column (c + j) % 32: all different): no
//     bank conflict on either side.  Those four words are a 4 x 4 block of bytes; it is transposed in registers, and the
//     four resulting words, each four bytes along a, go to four output rows.  Every global load and store is a word:
//     32 lanes x 4 B = one 128-B line per half-wave on both sides; single bytes only at the ragged edge of a volume.
// uint8 volumes may start at any byte and have any W: the word and 16-B accesses go through types of 1-B alignment (the
// fp32 ones through 4-B alignment, as in prep.hip).  Every index is 32-bit: N D H W < 2^31 is an argument check.
#include "common.h"

namespace effq {

constexpr int RO_THREADS = 256;
constexpr int RO_MAX_BLOCKS = 1 << 16;      // both kernels stride over their items

struct __attribute__((packed, aligned(4))) Vec16A4 { uint32_t v[4]; };    // 16 B at any 4-B boundary
struct __attribute__((packed, aligned(1))) Vec16A1 { uint32_t v[4]; };    // 16 B at any byte
struct __attribute__((packed, aligned(1))) WordA1 { uint32_t v; };        // 4 B at any byte

__device__ __forceinline__ uint32_t bswap(uint32_t v) { return __builtin_bswap32(v); }

// ---- variant 0 -------------------------------------------------------------------------------------------------------
struct RowsParams {
  const void* x;
  void* y;
  unsigned S;            // D H W
  unsigned O0, O1, W;    // output extents; the innermost is source W
  unsigned st0, st1;     // source strides (elements) of the source axes that became output axes 0 and 1
  unsigned gw;           // 16-B groups per row, ceil(W / VEC)
  unsigned total;        // N O0 O1 gw
  int flip;
};

template <typename E, typename V>
__global__ __launch_bounds__(RO_THREADS) void k_reorient_rows(RowsParams p) {
  constexpr unsigned VEC = 16 / sizeof(E);
  const E* x = static_cast<const E*>(p.x);
  E* y = static_cast<E*>(p.y);
  for (unsigned e = blockIdx.x * RO_THREADS + threadIdx.x; e < p.total; e += gridDim.x * RO_THREADS) {
    unsigned row = e / p.gw;
    const unsigned w0 = (e - row * p.gw) * VEC;
    const unsigned o1 = row % p.O1;
    row /= p.O1;
    const unsigned o0 = row % p.O0, n = row / p.O0;
    const unsigned c0 = (p.flip & 1) ? p.O0 - 1 - o0 : o0, c1 = (p.flip & 2) ? p.O1 - 1 - o1 : o1;
    const E* src = x + (n * p.S + c0 * p.st0 + c1 * p.st1);
    E* dst = y + ((n * p.O0 + o0) * p.O1 + o1) * p.W + w0;
    if (w0 + VEC <= p.W) {
      V v;
      if (p.flip & 4) {
        const V u = *reinterpret_cast<const V*>(src + (p.W - w0 - VEC));
        if (sizeof(E) == 4) {
          v.v[0] = u.v[3]; v.v[1] = u.v[2]; v.v[2] = u.v[1]; v.v[3] = u.v[0];
        } else {
          v.v[0] = bswap(u.v[3]); v.v[1] = bswap(u.v[2]); v.v[2] = bswap(u.v[1]); v.v[3] = bswap(u.v[0]);
        }
      } else {
        v = *reinterpret_cast<const V*>(src + w0);
      }
      *reinterpret_cast<V*>(dst) = v;
    } else {
      for (unsigned u = 0; w0 + u < p.W; ++u) dst[u] = (p.flip & 4) ? src[p.W - 1 - w0 - u] : src[w0 + u];
    }
  }
}

// ---- variant 1 -------------------------------------------------------------------------------------------------------
struct TileParams {
  const void* x;
  void* y;
  unsigned S;               // D H W
  unsigned A, B, W;         // source extents: a becomes output W, b is the other of D and H
  unsigned sa, sb;          // source strides of a and b (elements); source W has stride 1
  unsigned dw, db;          // output strides of the axes that source W and b became; a has stride 1
  unsigned nta, ntw;        // tiles along a and along W
  unsigned total;           // N B nta ntw
  int fa, fb, fw;           // the flips of the output axes that a, b and source W became
};

struct TileAt {
  unsigned src, dst, a0, w0;      // offsets of the plane (n, b) in x and in y; the tile's corner
};
__device__ __forceinline__ TileAt tile_at(const TileParams& p, unsigned t, unsigned ta_size, unsigned tw_size) {
  TileAt r;
  const unsigned tw = t % p.ntw;
  t /= p.ntw;
  const unsigned ta = t % p.nta;
  t /= p.nta;
  const unsigned ib = t % p.B, n = t / p.B;
  r.src = n * p.S + ib * p.sb;
  r.dst = n * p.S + (p.fb ? p.B - 1 - ib : ib) * p.db;
  r.a0 = ta * ta_size;
  r.w0 = tw * tw_size;
  return r;
}

constexpr int TF = 64;              // fp32 tile edge
__global__ __launch_bounds__(RO_THREADS) void k_reorient_tile_f32(TileParams p) {
  __shared__ uint32_t tile[TF][TF + 1];
  const uint32_t* x = static_cast<const uint32_t*>(p.x);
  uint32_t* y = static_cast<uint32_t*>(p.y);
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (unsigned t = blockIdx.x; t < p.total; t += gridDim.x) {
    const TileAt q = tile_at(p, t, TF, TF);
    const unsigned cw = q.w0 + lane;
#pragma unroll 4
    for (unsigned i = 0; i < TF / 4; ++i) {
      const unsigned r = i * 4 + wave, ia = q.a0 + r;
      if (ia < p.A && cw < p.W) tile[r][lane] = x[q.src + ia * p.sa + cw];
    }
    __syncthreads();
    const unsigned ia = q.a0 + lane;
    const unsigned ca = p.fa ? p.A - 1 - ia : ia;
#pragma unroll 4
    for (unsigned i = 0; i < TF / 4; ++i) {
      const unsigned r = i * 4 + wave, iw = q.w0 + r;
      if (iw < p.W && ia < p.A) y[q.dst + (p.fw ? p.W - 1 - iw : iw) * p.dw + ca] = tile[lane][r];
    }
    __syncthreads();
  }
}

constexpr int TB = 128;             // uint8 tile edge (bytes)
constexpr int TBW = TB / 4;         // words per tile row
__global__ __launch_bounds__(RO_THREADS) void k_reorient_tile_u8(TileParams p) {
  __shared__ uint32_t tile[TB * TBW];
  const uint8_t* x = static_cast<const uint8_t*>(p.x);
  uint8_t* y = static_cast<uint8_t*>(p.y);
  const unsigned half = (threadIdx.x >> 5) & 1, l32 = threadIdx.x & 31, wave = threadIdx.x >> 6;
  for (unsigned t = blockIdx.x; t < p.total; t += gridDim.x) {
    const TileAt q = tile_at(p, t, TB, TB);
    // phase 1: a half-wave loads the 32 words of one tile row; bytes past the volume are zero and never stored
    const unsigned cw = q.w0 + 4 * l32;
#pragma unroll 4
    for (unsigned i = 0; i < TB / 8; ++i) {
      const unsigned r = (i * 4 + wave) * 2 + half, ia = q.a0 + r;
      uint32_t v = 0;
      if (ia < p.A && cw < p.W) {
        const uint8_t* s = x + (q.src + ia * p.sa + cw);
        if (cw + 4 <= p.W) {
          v = reinterpret_cast<const WordA1*>(s)->v;
        } else {
          for (unsigned u = 0; cw + u < p.W; ++u) v |= (uint32_t)s[u] << (8 * u);
        }
      }
      tile[r * TBW + ((l32 + (r >> 2)) & (TBW - 1))] = v;
    }
    __syncthreads();
    // phase 2: lane j of a half takes the 4 x 4 bytes of rows 4 j ... 4 j + 3 and word c, transposes them, and stores one
    // word (four bytes along a) to each of the output rows 4 c ... 4 c + 3
    const unsigned ia = q.a0 + 4 * l32;
#pragma unroll 2
    for (unsigned i = 0; i < TBW / 8; ++i) {
      const unsigned c = (i * 4 + wave) * 2 + half;
      uint32_t r[4];
#pragma unroll
      for (unsigned k = 0; k < 4; ++k) r[k] = tile[(4 * l32 + k) * TBW + ((c + l32) & (TBW - 1))];
      if (ia >= p.A) continue;
      const unsigned na = min(4u, p.A - ia);      // bytes of this lane's words that lie inside the volume
#pragma unroll
      for (unsigned j = 0; j < 4; ++j) {
        const unsigned iw = q.w0 + 4 * c + j;
        if (iw >= p.W) break;
        uint32_t o = ((r[0] >> (8 * j)) & 0xffu) | (((r[1] >> (8 * j)) & 0xffu) << 8) |
                     (((r[2] >> (8 * j)) & 0xffu) << 16) | (((r[3] >> (8 * j)) & 0xffu) << 24);
        uint8_t* row = y + (q.dst + (p.fw ? p.W - 1 - iw : iw) * p.dw);
        if (na == 4) {
          if (p.fa) reinterpret_cast<WordA1*>(row + (p.A - 4 - ia))->v = bswap(o);
          else reinterpret_cast<WordA1*>(row + ia)->v = o;
        } else {
          for (unsigned u = 0; u < na; ++u) row[p.fa ? p.A - 1 - ia - u : ia + u] = (uint8_t)(o >> (8 * u));
        }
      }
    }
    __syncthreads();
  }
}

// the argument checks both entry points share; leaves the inverse permutation in inv[source axis] = output axis
static inline bool reorient_plan_ok(const int* src_axis, int flip_mask, int elem_bytes, int* inv) {
  if (!src_axis || flip_mask < 0 || flip_mask >= 8 || (elem_bytes != 1 && elem_bytes != 4)) return false;
  inv[0] = inv[1] = inv[2] = -1;
  for (int p = 0; p < 3; ++p) {
    if (src_axis[p] < 0 || src_axis[p] > 2 || inv[src_axis[p]] != -1) return false;
    inv[src_axis[p]] = p;
  }
  return true;
}

static inline unsigned reorient_grid(unsigned items) {
  return items < 1 ? 1u : (items > (unsigned)RO_MAX_BLOCKS ? (unsigned)RO_MAX_BLOCKS : items);
}

}  // namespace effq
using namespace effq;

extern "C" {

int effq_prep_reorient_plan(const int* src_axis, int flip_mask, int elem_bytes, int* variant) {
  int inv[3];
  EFFQ_CHECK_ARG(variant && reorient_plan_ok(src_axis, flip_mask, elem_bytes, inv));
  *variant = src_axis[2] == 2 ? 0 : 1;
  return EFFQ_OK;
}

int effq_prep_reorient(const void* x, int N, int D, int H, int W, const int* src_axis, int flip_mask, int elem_bytes,
                       void* y, void* stream) {
  int inv[3];
  EFFQ_CHECK_ARG(x && y && reorient_plan_ok(src_axis, flip_mask, elem_bytes, inv));
  EFFQ_CHECK_ARG(N > 0 && D > 0 && H > 0 && W > 0 && D <= 32767 && H <= 32767 && W <= 32767 &&
                 (long long)N * D * H * W < (1ll << 31));       // prep_fits of prep.hip
  const uintptr_t xb = reinterpret_cast<uintptr_t>(x), yb = reinterpret_cast<uintptr_t>(y);
  const uintptr_t bytes = (uintptr_t)N * D * H * W * (uintptr_t)elem_bytes;
  EFFQ_CHECK_ARG(xb % (uintptr_t)elem_bytes == 0 && yb % (uintptr_t)elem_bytes == 0);
  EFFQ_CHECK_ARG(xb + bytes <= yb || yb + bytes <= xb);         // x and y must not overlap
  const unsigned dims[3] = {(unsigned)D, (unsigned)H, (unsigned)W};
  const unsigned sstr[3] = {(unsigned)H * W, (unsigned)W, 1u};
  const unsigned od[3] = {dims[src_axis[0]], dims[src_axis[1]], dims[src_axis[2]]};
  const unsigned ostr[3] = {od[1] * od[2], od[2], 1u};
  const hipStream_t st = as_stream(stream);
  if (src_axis[2] == 2) {
    RowsParams p;
    p.x = x; p.y = y; p.S = (unsigned)D * H * W;
    p.O0 = od[0]; p.O1 = od[1]; p.W = (unsigned)W;
    p.st0 = sstr[src_axis[0]]; p.st1 = sstr[src_axis[1]];
    const unsigned vec = 16u / (unsigned)elem_bytes;
    p.gw = (p.W + vec - 1) / vec;
    p.total = (unsigned)N * p.O0 * p.O1 * p.gw;                 // at most N D H W
    p.flip = flip_mask;
    const dim3 g(reorient_grid((p.total + RO_THREADS - 1) / RO_THREADS)), b(RO_THREADS);
    if (elem_bytes == 4)
      hipLaunchKernelGGL((k_reorient_rows<uint32_t, Vec16A4>), g, b, 0, st, p);
    else
      hipLaunchKernelGGL((k_reorient_rows<uint8_t, Vec16A1>), g, b, 0, st, p);
  } else {
    const int a = src_axis[2], bx = 1 - a;                      // a, b: source D and H in the order the plan needs
    const unsigned edge = elem_bytes == 4 ? (unsigned)TF : (unsigned)TB;
    TileParams p;
    p.x = x; p.y = y; p.S = (unsigned)D * H * W;
    p.A = dims[a]; p.B = dims[bx]; p.W = (unsigned)W;
    p.sa = sstr[a]; p.sb = sstr[bx];
    p.dw = ostr[inv[2]]; p.db = ostr[inv[bx]];
    p.nta = (p.A + edge - 1) / edge; p.ntw = (p.W + edge - 1) / edge;
    p.total = (unsigned)N * p.B * p.nta * p.ntw;                // at most N D H W
    p.fa = (flip_mask >> 2) & 1; p.fb = (flip_mask >> inv[bx]) & 1; p.fw = (flip_mask >> inv[2]) & 1;
    const dim3 g(reorient_grid(p.total)), b(RO_THREADS);
    if (elem_bytes == 4)
      hipLaunchKernelGGL(k_reorient_tile_f32, g, b, 0, st, p);
    else
      hipLaunchKernelGGL(k_reorient_tile_u8, g, b, 0, st, p);
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // extern "C"
