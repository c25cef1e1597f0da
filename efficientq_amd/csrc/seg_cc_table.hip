// One record per connected component (effq_cc_table, effq_seg_lesion_table: validate_seg(..., lesion_table=True)): four
// launches after the labelling of seg_cc.hip (cc_run, through seg_cc.h), on the labels it leaves flattened.
#include "common.h"
#include "seg_cc.h"

namespace effq {

// ---- table ----------------------------------------------------------------------------------------------------------
// One row per component, in ascending order of its first voxel (scipy.ndimage.label's numbering), from the flattened
// labels of cc_run (labels[v] = root + 1, a root has labels[v] == v + 1):
//
//   chunks   the roots of every chunk of CC_CHUNK consecutive voxels are counted (ballots, no atomics)
//   scan     one workgroup per plane: exclusive scan of the chunk counts in place, the total is nrows
//   rank     every chunk is walked again: the k-th root of the plane gets row k = {first voxel, 0, 0} (k < max_rows) and
//            its own label word becomes -(k + 1), so a voxel finds its row through labels[labels[v] - 1]
//   accum    every foreground voxel adds 1 to the size of its row, and 1 to its overlap when both masks of its class
//            hold the voxel: equal rows of a wave are added once (the lane count), the sums of a workgroup are kept in
//            LDS slots and reach the table once per slot
//
// Integer adds only: equal inputs give equal bits.  A workgroup reads and writes the label words of its own chunk only
// (rank), and the accumulation runs in a launch of its own after it.
constexpr int CC_CHUNK_ITERS = CC_CHUNK / CC_THREADS;  // ballots per wave: a wave owns CC_CHUNK / CC_WAVES voxels in a row
constexpr int CC_SLOTS = 256;                          // accum: rows a workgroup keeps in LDS (direct-mapped)
constexpr int CC_MATCH_ROUNDS = 4;                     // accum: distinct rows of a wave that are combined by ballot
static_assert(CC_CHUNK % CC_THREADS == 0, "a chunk is a whole number of ballots per wave");

// WRITE false: chunks (P, gridDim.x) = the roots of each chunk.  WRITE true: chunks holds the exclusive scan; the roots
// get their rows and their negative label words.  rows (P, max_rows, stride) int32.
template <bool WRITE>
__global__ __launch_bounds__(CC_THREADS) void k_cc_rank(int* __restrict__ labels, int S, uint32_t* __restrict__ chunks,
                                                        int max_rows, int stride, int32_t* __restrict__ rows) {
  __shared__ uint32_t s_wave[CC_WAVES];
  const int plane = blockIdx.y;
  int* L = labels + (size_t)plane * S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * CC_CHUNK + (long long)wave * (CC_CHUNK / CC_WAVES);
  unsigned long long bal[CC_CHUNK_ITERS];
  uint32_t n = 0;
#pragma unroll
  for (int k = 0; k < CC_CHUNK_ITERS; ++k) {
    const long long v = base + k * 64 + lane;
    bal[k] = __ballot(v < S && L[v] == (int)v + 1);
    n += (uint32_t)__popcll(bal[k]);
  }
  if (lane == 0) s_wave[wave] = n;
  __syncthreads();
  const size_t slot = (size_t)plane * gridDim.x + blockIdx.x;
  if constexpr (!WRITE) {
    if (threadIdx.x == 0) {
      uint32_t s = 0;
      for (int w = 0; w < CC_WAVES; ++w) s += s_wave[w];
      chunks[slot] = s;
    }
  } else {
    uint32_t off = chunks[slot];
    for (int w = 0; w < wave; ++w) off += s_wave[w];
#pragma unroll
    for (int k = 0; k < CC_CHUNK_ITERS; ++k) {
      if ((bal[k] >> lane) & 1ull) {
        const int v = (int)(base + k * 64 + lane);
        const uint32_t r = off + (uint32_t)__popcll(bal[k] & ((1ull << lane) - 1ull));
        L[v] = -(int)r - 1;
        if (r < (uint32_t)max_rows) {
          int32_t* row = rows + ((size_t)plane * max_rows + r) * stride;
          row[0] = v;
          for (int j = 1; j < stride; ++j) row[j] = 0;
        }
      }
      off += (uint32_t)__popcll(bal[k]);
    }
  }
}

// one workgroup per plane: thread t owns a run of consecutive chunks, the runs are scanned in LDS
__global__ __launch_bounds__(CC_THREADS) void k_cc_scan(uint32_t* __restrict__ chunks, int nchunks,
                                                        long long* __restrict__ nrows) {
  __shared__ uint32_t s_sum[CC_THREADS];
  uint32_t* c = chunks + (size_t)blockIdx.x * nchunks;
  const int t = threadIdx.x;
  const int per = (nchunks + CC_THREADS - 1) / CC_THREADS;
  const int b0 = min(nchunks, t * per), b1 = min(nchunks, b0 + per);
  uint32_t sum = 0;
  for (int b = b0; b < b1; ++b) sum += c[b];
  s_sum[t] = sum;
  __syncthreads();
  for (int o = 1; o < CC_THREADS; o <<= 1) {
    const uint32_t add = t >= o ? s_sum[t - o] : 0u;
    __syncthreads();
    s_sum[t] += add;
    __syncthreads();
  }
  uint32_t run = s_sum[t] - sum;          // exclusive
  for (int b = b0; b < b1; ++b) {
    const uint32_t k = c[b];
    c[b] = run;
    run += k;
  }
  if (t == CC_THREADS - 1) nrows[blockIdx.x] = (long long)s_sum[t];
}

// bits null: sizes only (stride 2).  Else plane q < C is the predicted mask of class q, plane C + q its label mask, and
// row[2] counts the voxels that both hold.
__global__ __launch_bounds__(CC_THREADS) void k_cc_accum(const int* __restrict__ labels,
                                                         const uint16_t* __restrict__ bits, int C, int S, int max_rows,
                                                         int stride, int32_t* __restrict__ rows) {
  __shared__ int s_key[CC_SLOTS];
  __shared__ uint32_t s_size[CC_SLOTS], s_ovl[CC_SLOTS];
  const int plane = blockIdx.y;
  const int* L = labels + (size_t)plane * S;
  int32_t* T = rows + (size_t)plane * max_rows * stride;
  const int c = plane < C ? plane : plane - C;
  for (int k = threadIdx.x; k < CC_SLOTS; k += CC_THREADS) {
    s_key[k] = -1;
    s_size[k] = 0;
    s_ovl[k] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  // the trip count is the same for every lane of a wave: the ballots below need them all
  for (long long i0 = (long long)blockIdx.x * CC_THREADS; i0 < S; i0 += (long long)gridDim.x * CC_THREADS) {
    const long long i = i0 + threadIdx.x;
    int r = -1;                            // the row of this lane's voxel; -1: nothing to add
    bool both = false;
    if (i < S) {
      const int l = L[i];
      if (l != 0) {
        r = cc_row(L, l);
        if (r >= max_rows) r = -1;
        if (bits && r >= 0) {
          const uint32_t b = bits[i];
          both = ((b >> c) & (b >> (8 + c)) & 1u) != 0;
        }
      }
    }
    // what this lane adds: the leader of a group carries the group's counts, the overlap from the same group mask
    const unsigned long long mboth = __ballot(both);
    uint32_t dovl = 0;
    const uint32_t dsize = wave_match_count<CC_MATCH_ROUNDS>(r >= 0, (uint32_t)r, lane,
                                                             [&](unsigned long long m, bool leader) {
                                                               if (leader) dovl = (uint32_t)__popcll(m & mboth);
                                                               return true;
                                                             });
    if (dsize == 1) dovl = both ? 1u : 0u;  // a lane left over or a group of one: its own voxel
    if (dsize == 0) continue;
    const int s = r & (CC_SLOTS - 1);
    int k = s_key[s];
    if (k == -1) {
      k = atomicCAS(&s_key[s], -1, r);
      if (k == -1) k = r;
    }
    if (k == r) {
      atomicAdd(&s_size[s], dsize);
      if (dovl) atomicAdd(&s_ovl[s], dovl);
    } else {                               // the slot belongs to another row
      atomicAdd(&T[(size_t)r * stride + 1], (int)dsize);
      if (dovl) atomicAdd(&T[(size_t)r * stride + 2], (int)dovl);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < CC_SLOTS; k += CC_THREADS) {
    const int r = s_key[k];
    if (r < 0) continue;
    atomicAdd(&T[(size_t)r * stride + 1], (int)s_size[k]);
    if (s_ovl[k]) atomicAdd(&T[(size_t)r * stride + 2], (int)s_ovl[k]);
  }
}

// the four launches after cc_run; bits null: sizes only
int cc_table_run(const CcTableWs& t, const uint16_t* bits, int C, int P, int S, int max_rows, int stride, int32_t* rows,
                 long long* nrows, hipStream_t st) {
  const dim3 b(CC_THREADS), gc(t.nchunks, P);
  hipLaunchKernelGGL(k_cc_rank<false>, gc, b, 0, st, t.cc.labels, S, t.chunks, max_rows, stride, rows);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_scan, dim3(P), b, 0, st, t.chunks, t.nchunks, nrows);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_rank<true>, gc, b, 0, st, t.cc.labels, S, t.chunks, max_rows, stride, rows);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_accum, dim3(cc_grid(S, CC_STREAM_BLOCKS), P), b, 0, st, t.cc.labels, bits, C, S, max_rows,
                     stride, rows);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

}  // namespace effq
using namespace effq;

extern "C" {

size_t effq_cc_table_ws_bytes(int P, int D, int H, int W, int max_rows) {
  if (!cc_dims_ok(P, D, H, W) || max_rows <= 0) return 0;
  return cc_table_ws(nullptr, P, (size_t)D * H * W).bytes;
}

int effq_cc_table(const uint8_t* masks, int P, int D, int H, int W, int connectivity, int max_rows, int32_t* rows,
                  long long* nrows, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(masks && rows && nrows && ws && max_rows > 0);
  EFFQ_CHECK_ARG(cc_dims_ok(P, D, H, W));
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  const CcTableWs t = cc_table_ws(ws, P, (size_t)D * H * W);
  EFFQ_CHECK_WS(ws_bytes, t.bytes);
  const hipStream_t st = as_stream(stream);
  const int rc =
      cc_run(cc_src_masks(masks), P, D, H, W, connectivity, t.cc.labels, nullptr, 0, t.cc.partial, nrows, st);
  if (rc != EFFQ_OK) return rc;
  return cc_table_run(t, nullptr, 0, P, D * H * W, max_rows, 2, rows, nrows, st);
}

int effq_seg_lesion_table(const float* logits, const uint8_t* label, int C, int D, int H, int W, int mode, int fuse,
                          float thresh, int connectivity, int max_rows, long long* counts, long long* nrows,
                          int32_t* rows, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(logits && label && counts && nrows && rows && ws && max_rows > 0);
  EFFQ_CHECK_ARG(C > 0 && C <= EFFQ_SEG_TALLIES_MAX_CLASSES);
  EFFQ_CHECK_ARG(cc_dims_ok(2 * C, D, H, W));
  EFFQ_CHECK_ARG(mode == EFFQ_SEG_ARGMAX || mode == EFFQ_SEG_SIGMOID);
  EFFQ_CHECK_ARG(fuse == EFFQ_SEG_FUSE_NONE || fuse == EFFQ_SEG_FUSE_AGG || fuse == EFFQ_SEG_FUSE_CON);
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  const int P = 2 * C;
  const size_t S = (size_t)D * H * W;
  const CcTableWs t = cc_table_ws(ws, P, S);
  EFFQ_CHECK_WS(ws_bytes, t.bytes);
  const hipStream_t st = as_stream(stream);
  int rc = cc_decision_bits(logits, label, C, S, mode, fuse, thresh, t.cc.bits, st);
  if (rc != EFFQ_OK) return rc;
  rc = cc_run(cc_src_bits(t.cc.bits, C), P, D, H, W, connectivity, t.cc.labels, t.cc.flags, C, t.cc.partial, counts,
              st);
  if (rc != EFFQ_OK) return rc;
  return cc_table_run(t, t.cc.bits, C, P, (int)S, max_rows, 3, rows, nrows, st);
}

}  // extern "C"
