// What the prep kernels share (prep.hip, prep_smooth.hip, prep_quantile.hip, prep_align.hip): the launch shape, the 16-B
// vector of 4-B alignment, the mask, the item of four consecutive w of one row, and the argument checks of the extents and the pointers.
#pragma once
#include "common.h"

namespace effq {

constexpr int PREP_THREADS = 256;
constexpr int PREP_WAVES = PREP_THREADS / 64;
constexpr int PREP_MAX_BLOCKS = 1024;

struct __attribute__((packed, aligned(4))) PFloat4 { float x, y, z, w; };    // 16 B at any 4-B boundary
struct __attribute__((packed, aligned(1))) PByte4 { uint8_t x, y, z, w; };    // four labels at any byte

static inline unsigned prep_grid(size_t groups) {
  size_t nb = (groups + PREP_THREADS - 1) / PREP_THREADS;
  return (unsigned)(nb < 1 ? 1 : (nb > (size_t)PREP_MAX_BLOCKS ? (size_t)PREP_MAX_BLOCKS : nb));
}

// the mask of a modality: EFFQ_PREP_MASK_NONZERO (0) x != 0, a NaN inside; EFFQ_PREP_MASK_ALL every voxel
__device__ __forceinline__ bool in_mask(float v, int mask_mode) { return mask_mode != 0 || v != 0.0f; }

// A thread takes four consecutive w of one output row: gw = ceil(OW / 4) threads per row, rows = N * OD * OH.
struct RowItem {
  unsigned n, d, h, w0;
};
__device__ __forceinline__ RowItem row_item(unsigned e, unsigned gw, unsigned OD, unsigned OH) {
  RowItem r;
  unsigned row = e / gw;
  r.w0 = (e - row * gw) * 4;
  r.h = row % OH;
  row /= OH;
  r.d = row % OD;
  r.n = row / OD;
  return r;
}

static inline bool prep_fits(long long N, long long D, long long H, long long W) {
  return N > 0 && D > 0 && H > 0 && W > 0 && D <= 32767 && H <= 32767 && W <= 32767 && N * D * H * W < (1ll << 31);
}
static inline bool prep_fits_flat(long long C, long long S) { return C > 0 && S > 0 && S < (1ll << 31) && C * S < (1ll << 31); }
static inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace effq
