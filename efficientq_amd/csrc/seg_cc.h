// What the users of the connected-component labelling share: where the foreground of a plane comes from (CcSrc), the
// workspace of cc_run (CcWs) and cc_run itself, which seg_cc.hip defines.  Its users are the lesion counts (seg_cc.hip),
// the lesion table (seg_cc_table.hip), the lesion pairs (seg_cc_match.hip), which also share the table's workspace
// (CcTableWs), its launches (cc_table_run, defined in seg_cc_table.hip) and the row of a voxel (cc_row), and the rules
// of --post (label_post.hip).  No kernel lives here: the labelling kernels exist in seg_cc.o alone, the table's in
// seg_cc_table.o.
#pragma once
#include "common.h"
#include "seg_masks.h"

namespace effq {

constexpr int CC_WAVES = CC_THREADS / 64;
constexpr int CC_COUNT_BLOCKS = 512;                   // count: blocks per plane at most = partials per plane
constexpr int CC_CHUNK = EFFQ_CC_TABLE_CHUNK;          // table: the voxels of one chunk of the rank scan

// where the foreground of plane q comes from: P masks of uint8, or bit q of the decision bits (pred | gt << 8)
struct CcSrc {
  const uint8_t* masks;
  const uint16_t* bits;
  int C;
};
static inline CcSrc cc_src_masks(const uint8_t* masks) { return CcSrc{masks, nullptr, 0}; }
static inline CcSrc cc_src_bits(const uint16_t* bits, int C) { return CcSrc{nullptr, bits, C}; }

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

static bool cc_dims_ok(int P, int D, int H, int W) {
  return P > 0 && P <= 65535 && D > 0 && H > 0 && W > 0 && (long long)P * D * H * W < (1ll << 31);
}

// seg_cc.hip: the five launches after the masks, which leave labels flattened (labels[v] = root + 1, 0 for background);
// C == 0: plain labelling (no flags), out = ncomp (P)
int cc_run(const CcSrc& src, int P, int D, int H, int W, int conn, int* labels, uint8_t* flags, int C, uint32_t* partial,
           long long* out, hipStream_t st);

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

// seg_cc_table.hip: the four launches after cc_run, which leave the label word of the k-th root of a plane at -(k + 1);
// bits null: sizes only
int cc_table_run(const CcTableWs& t, const uint16_t* bits, int C, int P, int S, int max_rows, int stride, int32_t* rows,
                 long long* nrows, hipStream_t st);

#ifdef __HIPCC__
// the row of a foreground voxel after cc_table_run, from its label word l != 0 and the labels L of its plane
__device__ __forceinline__ int cc_row(const int* __restrict__ L, int l) { return l < 0 ? -l - 1 : -L[l - 1] - 1; }
#endif

}  // namespace effq
