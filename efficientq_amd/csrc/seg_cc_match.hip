// The overlap of every (label lesion, predicted lesion) pair of a class (effq_seg_lesion_match: validate_seg(...,
// lesion_match=True)): the launches of the lesion table (cc_run and cc_table_run, through seg_cc.h) and four more, on
// the labels they leave and the decision bits.
#include "common.h"
#include "seg_cc.h"

namespace effq {

// ---- match ----------------------------------------------------------------------------------------------------------
// A sparse contingency table of the predicted plane c and the label plane C + c.  The key of a voxel that both masks hold
// is (label row << 32) | predicted row, rows as k_cc_rank<true> numbers them (whether or not they fit max_rows):
//
//   init     the keys of the hash tables become MATCH_EMPTY, their counts and the three words of every class 0: the
//            workspace may hold anything on entry
//   pairs    one streaming pass per class: equal keys of a wave are added once (wave_match_count on the label row, the
//            group split by the predicted row), the sums of a workgroup are kept in direct-mapped LDS slots, and what is
//            left goes into the class's open-addressing table: a 64-bit atomicCAS claims a slot, an atomicAdd counts
//   compact  the occupied slots are gathered (one atomicAdd per wave), in any order
//   order    rank = the keys below mine; the keys are distinct, so out[rank] is a sort.  npairs is written here
//
// Integer adds only, and the order is that of the keys: equal inputs give equal bits whatever the scheduling.  The table
// holds 2 max_pairs slots or more.  The claim that finds max_pairs keys claimed before it sets the class's overflow
// word, after which nothing more of the class is inserted; a probe ends after one turn round the table and sets the
// word too.  No loop waits for another workgroup.
constexpr unsigned long long MATCH_EMPTY = ~0ull;      // no key: a row is below 2^31
constexpr int MATCH_SLOTS = 256;                       // pairs: keys a workgroup keeps in LDS (direct-mapped)
constexpr int MATCH_ROUNDS = 4;                        // pairs: distinct label rows of a wave that are combined by ballot
constexpr int MATCH_MIN_SLOTS = 256;                   // the least table: a whole number of workgroups
constexpr int MATCH_WORDS = 4;                         // per class: overflow, keys claimed, keys gathered, (spare)

struct MatchWs {
  CcTableWs table;
  uint32_t* words;            // (C, MATCH_WORDS)
  unsigned long long* keys;   // (C, slots)
  uint32_t* counts;           // (C, slots)
  unsigned long long* gkeys;  // (C, max_pairs): the keys gathered
  uint32_t* gcounts;          // (C, max_pairs)
  uint32_t slots;             // a power of two
  size_t bytes;
};

static bool match_dims_ok(int C, int max_pairs) {
  return max_pairs > 0 && (long long)C * max_pairs * 3 < (1ll << 31);
}

static MatchWs match_ws(void* ws, int C, size_t S, int max_pairs) {
  MatchWs r;
  r.table = cc_table_ws(ws, 2 * C, S);
  r.slots = MATCH_MIN_SLOTS;
  while (r.slots < 2u * (uint32_t)max_pairs) r.slots <<= 1;
  char* p = static_cast<char*>(ws);
  size_t off = r.table.bytes;
  r.words = reinterpret_cast<uint32_t*>(p + off);            off += align16((size_t)C * MATCH_WORDS * sizeof(uint32_t));
  r.keys = reinterpret_cast<unsigned long long*>(p + off);   off += align16((size_t)C * r.slots * sizeof(unsigned long long));
  r.counts = reinterpret_cast<uint32_t*>(p + off);           off += align16((size_t)C * r.slots * sizeof(uint32_t));
  r.gkeys = reinterpret_cast<unsigned long long*>(p + off);  off += align16((size_t)C * max_pairs * sizeof(unsigned long long));
  r.gcounts = reinterpret_cast<uint32_t*>(p + off);          off += align16((size_t)C * max_pairs * sizeof(uint32_t));
  r.bytes = off;
  return r;
}

__device__ __forceinline__ uint32_t match_hash(unsigned long long k) {   // the finaliser of MurmurHash3
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}

__global__ __launch_bounds__(CC_THREADS) void k_match_init(unsigned long long* __restrict__ keys,
                                                           uint32_t* __restrict__ counts, uint32_t* __restrict__ words,
                                                           long long nslots, int nwords) {
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < nslots;
       i += (long long)gridDim.x * CC_THREADS) {
    keys[i] = MATCH_EMPTY;
    counts[i] = 0;
    if (i < nwords) words[i] = 0;
  }
}

// `add` voxels of `key` into the table of a class: keys and counts of mask + 1 slots, w its MATCH_WORDS words
__device__ __forceinline__ void match_insert(unsigned long long* __restrict__ keys, uint32_t* __restrict__ counts,
                                             uint32_t mask, uint32_t* __restrict__ w, int max_pairs,
                                             unsigned long long key, uint32_t add) {
  if (__hip_atomic_load(&w[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;   // the class has overflowed
  uint32_t s = match_hash(key) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
    unsigned long long k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == MATCH_EMPTY) {
      k = atomicCAS(&keys[s], MATCH_EMPTY, key);
      if (k == MATCH_EMPTY) {                                // a new key: more than max_pairs of them is the overflow
        k = key;
        if (atomicAdd(&w[1], 1u) >= (uint32_t)max_pairs) atomicOr(&w[0], 1u);
      }
    }
    if (k == key) {
      atomicAdd(&counts[s], add);
      return;
    }
  }
  atomicOr(&w[0], 1u);                                       // once round a full table
}

__global__ __launch_bounds__(CC_THREADS) void k_match_pairs(const int* __restrict__ labels,
                                                            const uint16_t* __restrict__ bits, int C, int S,
                                                            unsigned long long* __restrict__ keys,
                                                            uint32_t* __restrict__ counts, uint32_t slots,
                                                            uint32_t* __restrict__ words, int max_pairs) {
  __shared__ unsigned long long s_key[MATCH_SLOTS];
  __shared__ uint32_t s_cnt[MATCH_SLOTS];
  const int c = blockIdx.y;
  const int* Lp = labels + (size_t)c * S;
  const int* Ll = labels + (size_t)(C + c) * S;
  unsigned long long* K = keys + (size_t)c * slots;
  uint32_t* N = counts + (size_t)c * slots;
  uint32_t* w = words + (size_t)c * MATCH_WORDS;
  const uint32_t mask = slots - 1;
  for (int k = threadIdx.x; k < MATCH_SLOTS; k += CC_THREADS) {
    s_key[k] = MATCH_EMPTY;
    s_cnt[k] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  // the trip count is the same for every lane of a wave: the ballots below need them all
  for (long long i0 = (long long)blockIdx.x * CC_THREADS; i0 < S; i0 += (long long)gridDim.x * CC_THREADS) {
    const long long i = i0 + threadIdx.x;
    bool both = false;
    uint32_t rl = 0, rp = 0;                 // the rows of this lane's voxel in the label and in the predicted plane
    if (i < S) {
      const uint32_t b = bits[i];
      both = ((b >> c) & (b >> (8 + c)) & 1u) != 0;
      if (both) {
        rl = (uint32_t)cc_row(Ll, Ll[i]);
        rp = (uint32_t)cc_row(Lp, Lp[i]);
      }
    }
    // what this lane adds at its key: the lanes of one label row form a group, those of them that share the leader's
    // predicted row are added once, by the leader; every other lane adds its own voxel
    uint32_t add = both ? 1u : 0u;
    wave_match_count<MATCH_ROUNDS>(both, rl, lane, [&](unsigned long long m, bool leader) {
      const int lead = __ffsll((long long)m) - 1;
      const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)rp, lead);
      const unsigned long long m2 = __ballot(rp == p) & m;
      if ((m2 >> lane) & 1ull) add = leader ? (uint32_t)__popcll(m2) : 0u;
      return true;
    });
    if (add == 0) continue;
    const unsigned long long key = ((unsigned long long)rl << 32) | rp;
    const int s = (int)((match_hash(key) >> 16) & (MATCH_SLOTS - 1));
    unsigned long long k = s_key[s];
    if (k == MATCH_EMPTY) {
      k = atomicCAS(&s_key[s], MATCH_EMPTY, key);
      if (k == MATCH_EMPTY) k = key;
    }
    if (k == key)
      atomicAdd(&s_cnt[s], add);
    else                                     // the slot belongs to another key
      match_insert(K, N, mask, w, max_pairs, key, add);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < MATCH_SLOTS; k += CC_THREADS)
    if (s_key[k] != MATCH_EMPTY) match_insert(K, N, mask, w, max_pairs, s_key[k], s_cnt[k]);
}

// one thread per slot (slots is a whole number of workgroups): the occupied slots of a wave take their places with one add
__global__ __launch_bounds__(CC_THREADS) void k_match_compact(const unsigned long long* __restrict__ keys,
                                                              const uint32_t* __restrict__ counts, uint32_t slots,
                                                              uint32_t* __restrict__ words, int max_pairs,
                                                              unsigned long long* __restrict__ gkeys,
                                                              uint32_t* __restrict__ gcounts) {
  const int c = blockIdx.y;
  const size_t s = (size_t)c * slots + (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const unsigned long long key = keys[s];
  const unsigned long long m = __ballot(key != MATCH_EMPTY);
  if (m == 0) return;
  const int lead = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if (lane == lead) base = atomicAdd(&words[(size_t)c * MATCH_WORDS + 2], (uint32_t)__popcll(m));
  base = (uint32_t)__builtin_amdgcn_readlane((int)base, lead);
  if (key == MATCH_EMPTY) return;
  const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (at < (uint32_t)max_pairs) {
    gkeys[(size_t)c * max_pairs + at] = key;
    gcounts[(size_t)c * max_pairs + at] = counts[s];
  }
}

// npairs (C), pairs (C, max_pairs, 3) = label row, predicted row, voxels of both, ascending in the key
__global__ __launch_bounds__(CC_THREADS) void k_match_order(const unsigned long long* __restrict__ gkeys,
                                                            const uint32_t* __restrict__ gcounts,
                                                            const uint32_t* __restrict__ words, int max_pairs,
                                                            long long* __restrict__ npairs, int32_t* __restrict__ pairs) {
  __shared__ unsigned long long s_key[CC_THREADS];
  const int c = blockIdx.y;
  const uint32_t* w = words + (size_t)c * MATCH_WORDS;
  const uint32_t n = w[2];
  const bool over = w[0] != 0 || n > (uint32_t)max_pairs;
  if (blockIdx.x == 0 && threadIdx.x == 0) npairs[c] = over ? -1ll : (long long)n;
  if (over || (uint32_t)blockIdx.x * CC_THREADS >= n) return;     // the same for the whole workgroup
  const unsigned long long* G = gkeys + (size_t)c * max_pairs;
  const uint32_t i = (uint32_t)blockIdx.x * CC_THREADS + threadIdx.x;
  const unsigned long long mine = i < n ? G[i] : MATCH_EMPTY;
  uint32_t rank = 0;
  for (uint32_t t0 = 0; t0 < n; t0 += CC_THREADS) {
    s_key[threadIdx.x] = t0 + threadIdx.x < n ? G[t0 + threadIdx.x] : MATCH_EMPTY;   // no key lies above MATCH_EMPTY
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < CC_THREADS; ++j) rank += s_key[j] < mine ? 1u : 0u;
    __syncthreads();
  }
  if (i < n) {                               // rank < n <= max_pairs: n distinct keys
    int32_t* out = pairs + ((size_t)c * max_pairs + rank) * 3;
    out[0] = (int32_t)(mine >> 32);
    out[1] = (int32_t)(mine & 0xffffffffull);
    out[2] = (int32_t)gcounts[(size_t)c * max_pairs + i];
  }
}

// the four launches after cc_table_run
static int match_run(const MatchWs& m, int C, int S, int max_pairs, long long* npairs, int32_t* pairs, hipStream_t st) {
  const dim3 b(CC_THREADS);
  const long long nslots = (long long)C * m.slots;
  hipLaunchKernelGGL(k_match_init, dim3(cc_grid((size_t)nslots, CC_STREAM_BLOCKS)), b, 0, st, m.keys, m.counts, m.words,
                     nslots, C * MATCH_WORDS);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_match_pairs, dim3(cc_grid(S, CC_STREAM_BLOCKS), C), b, 0, st, m.table.cc.labels, m.table.cc.bits, C,
                     S, m.keys, m.counts, m.slots, m.words, max_pairs);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_match_compact, dim3(m.slots / CC_THREADS, C), b, 0, st, m.keys, m.counts, m.slots, m.words,
                     max_pairs, m.gkeys, m.gcounts);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_match_order, dim3((max_pairs + CC_THREADS - 1) / CC_THREADS, C), b, 0, st, m.gkeys, m.gcounts,
                     m.words, max_pairs, npairs, pairs);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // namespace effq
using namespace effq;

extern "C" {

size_t effq_seg_lesion_match_ws_bytes(int C, int D, int H, int W, int max_rows, int max_pairs) {
  if (C <= 0 || C > EFFQ_SEG_TALLIES_MAX_CLASSES || !cc_dims_ok(2 * C, D, H, W) || max_rows <= 0 ||
      !match_dims_ok(C, max_pairs))
    return 0;
  return match_ws(nullptr, C, (size_t)D * H * W, max_pairs).bytes;
}

int effq_seg_lesion_match(const float* logits, const uint8_t* label, int C, int D, int H, int W, int mode, int fuse,
                          float thresh, int connectivity, int max_rows, int max_pairs, long long* counts,
                          long long* nrows, int32_t* rows, long long* npairs, int32_t* pairs, void* ws, size_t ws_bytes,
                          void* stream) {
  EFFQ_CHECK_ARG(logits && label && counts && nrows && rows && npairs && pairs && ws && max_rows > 0);
  EFFQ_CHECK_ARG(C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(cc_dims_ok(2 * C, D, H, W));
  EFFQ_CHECK_ARG(mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID);
  EFFQ_CHECK_ARG(fuse == EFFQ_SEG_FUSE_NONE || fuse == EFFQ_SEG_FUSE_AGG || fuse == EFFQ_SEG_FUSE_CON);
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  EFFQ_CHECK_ARG(match_dims_ok(C, max_pairs));
  const int P = 2 * C;
  const size_t S = (size_t)D * H * W;
  const MatchWs m = match_ws(ws, C, S, max_pairs);
  EFFQ_CHECK_WS(ws_bytes, m.bytes);
  const CcTableWs& t = m.table;
  const hipStream_t st = as_stream(stream);
  int rc = cc_decision_bits(logits, label, C, S, mode, fuse, thresh, t.cc.bits, st);
  if (rc != EFFQ_OK) return rc;
  rc = cc_run(cc_src_bits(t.cc.bits, C), P, D, H, W, connectivity, t.cc.labels, t.cc.flags, C, t.cc.partial, counts,
              st);
  if (rc != EFFQ_OK) return rc;
  rc = cc_table_run(t, t.cc.bits, C, P, (int)S, max_rows, 3, rows, nrows, st);
  if (rc != EFFQ_OK) return rc;
  return match_run(m, C, (int)S, max_pairs, npairs, pairs, st);
}

}  // extern "C"
