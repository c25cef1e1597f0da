// The rules of --post on a uint8 label map, on the connected components of seg_cc.hip (cc_run, through seg_cc.h):
//
//   clean    (effq_label_clean) the components of a label map's values sized at their roots and the small or losing ones
//            relabelled: see "clean" below
//   post     (effq_label_post) the same rules, and holes filled and masks closed or opened by a ball, the latter through
//            the distance transform of seg_surf.h: see "post" below
#include "common.h"
#include "seg_cc.h"
#include "seg_surf.h"

namespace effq {

constexpr int CLEAN_MATCH_ROUNDS = 4;                  // sizes: distinct roots of a wave that are combined by ballot

// ---- clean ----------------------------------------------------------------------------------------------------------
// effq_label_clean: the rules of --post on a uint8 label map, one after the other on the map the previous rule left.  Per
// rule, after the five launches of cc_run on the plane "the voxel's value is in the rule's set":
//
//   mask     (before cc_run) the membership of every voxel -> one 0/1 plane; the size words are zeroed in the same pass
//   sizes    every foreground voxel adds 1 to the size word of its root: equal roots of a wave are added once (the lane
//            count), as k_cc_accum does
//   best     (largest only) every root offers size << 32 | (0xFFFFFFFF - root) to one 64-bit atomicMax: the largest size
//            wins, and of equal sizes the least root (the component whose first voxel comes first)
//   apply    the voxels of a losing (largest) or small (min) component become TO and are counted
//
// Integer adds and one max only: equal inputs give equal bits.  The map is rewritten in place (`out`, a copy of `in` when
// they differ): a voxel is written by the thread that read it, and the labels of a rule are complete before its apply.
struct CleanSet {
  unsigned long long w[4];   // bit v set: the value v is in the rule's mask
};

struct CleanWs {
  uint32_t* partial;             // (CC_COUNT_BLOCKS, 2): cc_run's
  int* labels;                   // (S)
  int* sizes;                    // (S): the voxels of a component, at its root
  uint8_t* mask;                 // (S)
  unsigned long long* best;      // (EFFQ_LABEL_CLEAN_MAX_RULES)
  size_t bytes;
};

static CleanWs clean_ws(void* ws, size_t S) {
  CleanWs r;
  char* p = static_cast<char*>(ws);
  size_t off = 0;
  r.partial = reinterpret_cast<uint32_t*>(p + off); off += align16((size_t)CC_COUNT_BLOCKS * 2 * sizeof(uint32_t));
  r.labels = reinterpret_cast<int*>(p + off);       off += align16(S * sizeof(int));
  r.sizes = reinterpret_cast<int*>(p + off);        off += align16(S * sizeof(int));
  r.mask = reinterpret_cast<uint8_t*>(p + off);     off += align16(S);
  r.best = reinterpret_cast<unsigned long long*>(p + off);
  off += align16(EFFQ_LABEL_CLEAN_MAX_RULES * sizeof(unsigned long long));
  r.bytes = off;
  return r;
}

// stats (R, 2) and best (R) start at 0: the relabelled voxels and the counts of effq_label_post's rules are added to;
// the components of a largest / min rule are written over the first word by k_cc_final
__global__ __launch_bounds__(64) void k_clean_init(unsigned long long* __restrict__ best, long long* __restrict__ stats,
                                                   int R) {
  const int r = threadIdx.x;
  if (r >= R) return;
  best[r] = 0ull;
  stats[2 * r] = 0;
  stats[2 * r + 1] = 0;
}

__global__ __launch_bounds__(CC_THREADS) void k_clean_mask(const uint8_t* __restrict__ map, CleanSet set, int S,
                                                           uint8_t* __restrict__ mask, int* __restrict__ sizes) {
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const uint32_t v = map[i];
    mask[i] = (uint8_t)((set.w[v >> 6] >> (v & 63u)) & 1ull);
    sizes[i] = 0;
  }
}

// labels: flattened (labels[v] = root + 1, 0 for background)
__global__ __launch_bounds__(CC_THREADS) void k_clean_sizes(const int* __restrict__ labels, int S,
                                                            int* __restrict__ sizes) {
  const int lane = threadIdx.x & 63;
  // the trip count is the same for every lane of a wave: the ballots below need them all
  for (long long i0 = (long long)blockIdx.x * CC_THREADS; i0 < S; i0 += (long long)gridDim.x * CC_THREADS) {
    const long long i = i0 + threadIdx.x;
    const int r = i < S ? labels[i] - 1 : -1;      // the root of this lane's voxel; -1: nothing to add
    const int add = (int)wave_match_count<CLEAN_MATCH_ROUNDS>(r >= 0, (uint32_t)r, lane);
    if (add) atomicAdd(&sizes[r], add);
  }
}

__global__ __launch_bounds__(CC_THREADS) void k_clean_best(const int* __restrict__ labels,
                                                           const int* __restrict__ sizes, int S,
                                                           unsigned long long* __restrict__ best) {
  unsigned long long key = 0ull;
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)i;
    if (labels[v] != v + 1) continue;
    const unsigned long long k = ((unsigned long long)(uint32_t)sizes[v] << 32) | (0xFFFFFFFFull - (uint32_t)v);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0 && key) atomicMax(best, key);
}

// OP LARGEST: every component but the winner of `best` loses; OP MIN: every component of fewer than n voxels does
template <int OP>
__global__ __launch_bounds__(CC_THREADS) void k_clean_apply(const int* __restrict__ labels,
                                                            const int* __restrict__ sizes,
                                                            const unsigned long long* __restrict__ best, long long n,
                                                            int to, int S, uint8_t* __restrict__ map,
                                                            unsigned long long* __restrict__ changed) {
  int keep = -1;
  if constexpr (OP == EFFQ_LABEL_CLEAN_LARGEST) keep = (int)(0xFFFFFFFFu - (uint32_t)(*best & 0xFFFFFFFFull));
  uint32_t cnt = 0;
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const int l = labels[i];
    if (l == 0) continue;
    const bool lose = OP == EFFQ_LABEL_CLEAN_LARGEST ? l - 1 != keep : (long long)sizes[l - 1] < n;
    if (lose) {
      map[i] = (uint8_t)to;
      ++cnt;
    }
  }
  __shared__ uint32_t red[CC_WAVES];
  cnt = wave_sum_all(cnt);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < CC_WAVES; ++w) s += red[w];
    if (s) atomicAdd(changed, (unsigned long long)s);
  }
}

// one rule of effq_label_clean on the map `out`: 8 launches for MIN, 9 for LARGEST.  rule = op, N, TO (checked);
// stats (2) = components (written by k_cc_final), relabelled voxels (added to); best: the rule's word, zero before
static int clean_rule_run(const CleanWs& s, const CleanSet& set, const long long* rule, int D, int H, int W,
                          int connectivity, uint8_t* out, long long* stats, unsigned long long* best, hipStream_t st) {
  const int S = D * H * W;
  const dim3 b(CC_THREADS), gs(cc_grid((size_t)S, CC_STREAM_BLOCKS));
  const long long n = rule[1];
  const int to = (int)rule[2];
  unsigned long long* changed = reinterpret_cast<unsigned long long*>(stats + 1);
  hipLaunchKernelGGL(k_clean_mask, gs, b, 0, st, out, set, S, s.mask, s.sizes);
  EFFQ_LAUNCH_CHECK();
  const int rc = cc_run(cc_src_masks(s.mask), 1, D, H, W, connectivity, s.labels, nullptr, 0, s.partial, stats, st);
  if (rc != EFFQ_OK) return rc;
  hipLaunchKernelGGL(k_clean_sizes, gs, b, 0, st, s.labels, S, s.sizes);
  EFFQ_LAUNCH_CHECK();
  if (rule[0] == EFFQ_LABEL_CLEAN_LARGEST) {
    hipLaunchKernelGGL(k_clean_best, gs, b, 0, st, s.labels, s.sizes, S, best);
    EFFQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_clean_apply<EFFQ_LABEL_CLEAN_LARGEST>, gs, b, 0, st, s.labels, s.sizes, best, n, to, S, out,
                       changed);
  } else {
    hipLaunchKernelGGL(k_clean_apply<EFFQ_LABEL_CLEAN_MIN>, gs, b, 0, st, s.labels, s.sizes, best, n, to, S, out,
                       changed);
  }
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// ---- post -----------------------------------------------------------------------------------------------------------
// effq_label_post: the rules of effq_label_clean (clean_rule_run above, the same launches) and three morphological ones,
// on the mask M = "the voxel's value is in the rule's set" of the map the previous rule left.
//
//   fill     the complement of M is labelled at the dual connectivity (cc_run), every complement voxel on a face of the
//            volume marks its root (plain stores of 1), and the voxels of the unmarked components - the holes - become TO
//            and are counted, the roots among them as holes: 8 launches
//   close    M is written into a plane padded by R background voxels on every side, the exact distance transform of
//            seg_surf.h runs on it, a threshold writes the complement of the dilation {sq <= R^2} as the sites of a second
//            transform, and the voxels outside M whose second distance exceeds R^2 - the erosion of the dilation - become
//            TO: a memset and 9 launches
//   open     the same skeleton from the complement of M with the pad as sites: the first threshold is the erosion, the
//            voxels of M further than R from it become TO
//
// The pad makes both transforms those of the infinite grid with background outside the volume: a voxel outside the padded
// plane is more than R away from every voxel of the volume.  A plane without sites is INT32_MAX throughout, which the
// thresholds read as "further than R".  Integer compares and adds only: equal inputs give equal bits.
struct PostWs {
  CleanWs clean;                 // first: with max_radius 0 the workspace is effq_label_clean's and the words below
  long long* ncomp;              // (2): cc_run's component count of a fill rule (not reported)
  uint8_t* site;                 // (Sp): the sites of the padded plane
  int* sq;                       // (Sp): its squared distances
  size_t bytes;
};

static bool post_dims_ok(int D, int H, int W, int max_radius) {
  if (!cc_dims_ok(1, D, H, W) || max_radius < 0 || max_radius > EFFQ_LABEL_POST_MAX_RADIUS) return false;
  if (max_radius == 0) return true;
  const long long p = 2ll * max_radius;
  if (D + p > INT32_MAX || H + p > INT32_MAX || W + p > INT32_MAX) return false;
  return edt_dims_ok(1, (int)(D + p), (int)(H + p), (int)(W + p));
}

static PostWs post_ws(void* ws, int D, int H, int W, int max_radius) {
  PostWs r;
  r.clean = clean_ws(ws, (size_t)D * H * W);
  char* p = static_cast<char*>(ws);
  size_t off = r.clean.bytes;
  const size_t Sp = max_radius ? (size_t)(D + 2 * max_radius) * (H + 2 * max_radius) * (W + 2 * max_radius) : 0;
  r.ncomp = reinterpret_cast<long long*>(p + off); off += align16(2 * sizeof(long long));
  r.site = reinterpret_cast<uint8_t*>(p + off);    off += align16(Sp);
  r.sq = reinterpret_cast<int*>(p + off);          off += align16(Sp * sizeof(int));
  r.bytes = off;
  return r;
}

__device__ __forceinline__ bool clean_has(const CleanSet& set, uint32_t v) {
  return (set.w[v >> 6] >> (v & 63u)) & 1ull;
}

// two counts of a workgroup, each added by one 64-bit atomic (none for a zero)
__device__ __forceinline__ void post_add2(uint32_t a, uint32_t b, long long* dst) {
  __shared__ uint32_t red[CC_WAVES][2];
  a = wave_sum_all(a);
  b = wave_sum_all(b);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = a;
    red[threadIdx.x >> 6][1] = b;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    uint32_t s = 0;
    for (int w = 0; w < CC_WAVES; ++w) s += red[w][threadIdx.x];
    if (s) atomicAdd(reinterpret_cast<unsigned long long*>(dst) + threadIdx.x, (unsigned long long)s);
  }
}

// fill: k_clean_mask with the test inverted - the complement plane, and the root marks zeroed.  VEC 4: map 4-B aligned
template <int VEC>
__global__ __launch_bounds__(CC_THREADS) void k_post_comp_mask(const uint8_t* __restrict__ map, CleanSet set, int S,
                                                               uint8_t* __restrict__ mask, int* __restrict__ marks) {
  const long long tid = (long long)blockIdx.x * CC_THREADS + threadIdx.x, step = (long long)gridDim.x * CC_THREADS;
  const long long groups = S / VEC;
  for (long long g = tid; g < groups; g += step) {
    if constexpr (VEC == 4) {
      const uchar4 v = *reinterpret_cast<const uchar4*>(map + 4 * g);
      *reinterpret_cast<uchar4*>(mask + 4 * g) =
          make_uchar4(!clean_has(set, v.x), !clean_has(set, v.y), !clean_has(set, v.z), !clean_has(set, v.w));
      *reinterpret_cast<int4*>(marks + 4 * g) = make_int4(0, 0, 0, 0);
    } else {
      mask[g] = (uint8_t)!clean_has(set, map[g]);
      marks[g] = 0;
    }
  }
  const long long i = groups * VEC + tid;          // the last S % VEC voxels one by one
  if (i < S) {
    mask[i] = (uint8_t)!clean_has(set, map[i]);
    marks[i] = 0;
  }
}

// fill: the voxels on the six faces, 2 (H W + D W + D H) of them (an edge voxel comes twice: the store is the same).
// labels: flattened, of the complement plane
__global__ __launch_bounds__(CC_THREADS) void k_post_faces(const int* __restrict__ labels, int D, int H, int W,
                                                           int* __restrict__ marks) {
  const long long HW = (long long)H * W, DW = (long long)D * W, DH = (long long)D * H;
  const long long total = 2 * (HW + DW + DH);
  for (long long f = (long long)blockIdx.x * CC_THREADS + threadIdx.x; f < total; f += (long long)gridDim.x * CC_THREADS) {
    long long v;
    if (f < 2 * HW) {
      v = (f < HW ? 0 : (D - 1) * HW) + f % HW;
    } else if (f < 2 * (HW + DW)) {
      const long long g = f - 2 * HW, rem = g % DW;
      v = ((rem / W) * H + (g < DW ? 0 : H - 1)) * W + rem % W;
    } else {
      const long long g = f - 2 * (HW + DW);
      v = (g % DH) * W + (g < DH ? 0 : W - 1);
    }
    const int l = labels[v];
    if (l) marks[l - 1] = 1;
  }
}

// fill: stats (2) = holes (roots without a mark), voxels relabelled
__global__ __launch_bounds__(CC_THREADS) void k_post_fill_apply(const int* __restrict__ labels,
                                                                const int* __restrict__ marks, int to, int S,
                                                                uint8_t* __restrict__ map, long long* __restrict__ stats) {
  uint32_t holes = 0, cnt = 0;
  for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < S; i += (long long)gridDim.x * CC_THREADS) {
    const int l = labels[i];
    if (l == 0 || marks[l - 1] != 0) continue;
    map[i] = (uint8_t)to;
    ++cnt;
    if (l == (int)i + 1) ++holes;
  }
  post_add2(holes, cnt, stats);
}

// close / open: the sites of the volume's voxels inside the padded plane (the pad is a memset): M for close, its
// complement for open.  VEC 4: W % 4 == 0 and map 4-B aligned, so a group of four lies in one row
template <bool OPEN, int VEC>
__global__ __launch_bounds__(CC_THREADS) void k_post_sites(const uint8_t* __restrict__ map, CleanSet set, int S, int H,
                                                           int W, int rad, uint8_t* __restrict__ site) {
  const int Hp = H + 2 * rad, Wp = W + 2 * rad;
  const long long groups = S / VEC;                  // VEC 1 or S % 4 == 0
  for (long long g = (long long)blockIdx.x * CC_THREADS + threadIdx.x; g < groups; g += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)(g * VEC);
    const int w = v % W, q = v / W, h = q % H, d = q / H;
    uint8_t* dst = site + ((size_t)(d + rad) * Hp + h + rad) * Wp + w + rad;
    if constexpr (VEC == 4) {
      const uchar4 m = *reinterpret_cast<const uchar4*>(map + v);
      dst[0] = (uint8_t)(clean_has(set, m.x) != OPEN);
      dst[1] = (uint8_t)(clean_has(set, m.y) != OPEN);
      dst[2] = (uint8_t)(clean_has(set, m.z) != OPEN);
      dst[3] = (uint8_t)(clean_has(set, m.w) != OPEN);
    } else {
      dst[0] = (uint8_t)(clean_has(set, map[v]) != OPEN);
    }
  }
}

// close / open: the sites of the second transform, sq > R^2, over the whole padded plane (16-B loads, 4-B stores)
__global__ __launch_bounds__(CC_THREADS) void k_post_thresh(const int* __restrict__ sq, int Sp, int r2,
                                                            uint8_t* __restrict__ site) {
  const long long tid = (long long)blockIdx.x * CC_THREADS + threadIdx.x, step = (long long)gridDim.x * CC_THREADS;
  const long long groups = Sp / 4;
  for (long long g = tid; g < groups; g += step) {
    const int4 v = *reinterpret_cast<const int4*>(sq + 4 * g);
    *reinterpret_cast<uchar4*>(site + 4 * g) = make_uchar4(v.x > r2, v.y > r2, v.z > r2, v.w > r2);
  }
  const long long i = groups * 4 + tid;
  if (i < Sp) site[i] = (uint8_t)(sq[i] > r2);
}

// close: the voxels outside M with sq > R^2 become TO; open: the voxels of M with sq > R^2.  stats (2) = voxels of M
// before the rule, voxels relabelled.  VEC as k_post_sites
template <bool OPEN, int VEC>
__global__ __launch_bounds__(CC_THREADS) void k_post_ball_apply(const int* __restrict__ sq, CleanSet set, int S, int H,
                                                                int W, int rad, int r2, int to,
                                                                uint8_t* __restrict__ map, long long* __restrict__ stats) {
  const int Hp = H + 2 * rad, Wp = W + 2 * rad;
  const long long groups = S / VEC;
  uint32_t inside = 0, cnt = 0;
  for (long long g = (long long)blockIdx.x * CC_THREADS + threadIdx.x; g < groups; g += (long long)gridDim.x * CC_THREADS) {
    const int v = (int)(g * VEC);
    const int w = v % W, q = v / W, h = q % H, d = q / H;
    const int* e = sq + ((size_t)(d + rad) * Hp + h + rad) * Wp + w + rad;
    uint8_t m[VEC];
    if constexpr (VEC == 4) {
      const uchar4 u = *reinterpret_cast<const uchar4*>(map + v);
      m[0] = u.x; m[1] = u.y; m[2] = u.z; m[3] = u.w;
    } else {
      m[0] = map[v];
    }
    uint32_t hit = 0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const bool in = clean_has(set, m[k]);
      inside += in;
      if (in == OPEN && e[k] > r2) {
        m[k] = (uint8_t)to;
        ++hit;
      }
    }
    if (hit) {
      if constexpr (VEC == 4) *reinterpret_cast<uchar4*>(map + v) = make_uchar4(m[0], m[1], m[2], m[3]);
      else map[v] = m[0];
      cnt += hit;
    }
  }
  post_add2(inside, cnt, stats);
}

static inline bool post_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// fill on the map `out`: 8 launches.  dual: the connectivity of the holes
static int post_fill_run(const PostWs& s, const CleanSet& set, int to, int D, int H, int W, int dual, uint8_t* out,
                         long long* stats, hipStream_t st) {
  const int S = D * H * W;
  const CleanWs& c = s.clean;
  const dim3 b(CC_THREADS), gs(cc_grid((size_t)S, CC_STREAM_BLOCKS));
  int* marks = c.sizes;
  if (post_aligned4(out))
    hipLaunchKernelGGL(k_post_comp_mask<4>, dim3(cc_grid((size_t)S / 4 + 1, CC_STREAM_BLOCKS)), b, 0, st, out, set, S,
                       c.mask, marks);
  else
    hipLaunchKernelGGL(k_post_comp_mask<1>, gs, b, 0, st, out, set, S, c.mask, marks);
  EFFQ_LAUNCH_CHECK();
  const int rc = cc_run(cc_src_masks(c.mask), 1, D, H, W, dual, c.labels, nullptr, 0, c.partial, s.ncomp, st);
  if (rc != EFFQ_OK) return rc;
  const size_t faces = 2 * ((size_t)H * W + (size_t)D * W + (size_t)D * H);
  hipLaunchKernelGGL(k_post_faces, dim3(cc_grid(faces, CC_STREAM_BLOCKS)), b, 0, st, c.labels, D, H, W, marks);
  EFFQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_post_fill_apply, gs, b, 0, st, c.labels, marks, to, S, out, stats);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// close (OPEN false) or open of radius rad on the map `out`: a memset and 9 launches
template <bool OPEN>
static int post_ball_run(const PostWs& s, const CleanSet& set, int rad, int to, int D, int H, int W, uint8_t* out,
                         long long* stats, hipStream_t st) {
  const int S = D * H * W, r2 = rad * rad;
  const int Dp = D + 2 * rad, Hp = H + 2 * rad, Wp = W + 2 * rad, Sp = Dp * Hp * Wp;
  const dim3 b(CC_THREADS);
  const bool v4 = W % 4 == 0 && post_aligned4(out);
  const dim3 gs(cc_grid(v4 ? (size_t)S / 4 : (size_t)S, CC_STREAM_BLOCKS));
  EdtSrc src;
  src.masks = s.site; src.surf = nullptr; src.C = 0;
  EFFQ_HIP(hipMemsetAsync(s.site, OPEN ? 1 : 0, (size_t)Sp, st));
  if (v4) hipLaunchKernelGGL((k_post_sites<OPEN, 4>), gs, b, 0, st, out, set, S, H, W, rad, s.site);
  else hipLaunchKernelGGL((k_post_sites<OPEN, 1>), gs, b, 0, st, out, set, S, H, W, rad, s.site);
  EFFQ_LAUNCH_CHECK();
  int rc = edt_run<EdtVox>(src, 1, Dp, Hp, Wp, EdtUnit{}, EdtUnit{}, EdtUnit{}, s.sq, st);
  if (rc != EFFQ_OK) return rc;
  hipLaunchKernelGGL(k_post_thresh, dim3(cc_grid((size_t)Sp / 4 + 1, CC_STREAM_BLOCKS)), b, 0, st, s.sq, Sp, r2, s.site);
  EFFQ_LAUNCH_CHECK();
  rc = edt_run<EdtVox>(src, 1, Dp, Hp, Wp, EdtUnit{}, EdtUnit{}, EdtUnit{}, s.sq, st);
  if (rc != EFFQ_OK) return rc;
  if (v4) hipLaunchKernelGGL((k_post_ball_apply<OPEN, 4>), gs, b, 0, st, s.sq, set, S, H, W, rad, r2, to, out, stats);
  else hipLaunchKernelGGL((k_post_ball_apply<OPEN, 1>), gs, b, 0, st, s.sq, set, S, H, W, rad, r2, to, out, stats);
  EFFQ_LAUNCH_CHECK();
  return EFFQ_OK;
}

// The rule list of both entry points: rule r = op, N, TO in rules (R, 3), the values of its mask in sets (R, 256) ->
// set[r], and the largest radius of a close / open rule.  last_op: the ops up to it are allowed (effq_label_clean stops
// at MIN).  Which side of the mask TO lies on follows from the op, so the allowed ops are the only difference.
static int post_parse_rules(int R, const uint8_t* sets, const long long* rules, long long last_op, CleanSet* set,
                            int* max_radius) {
  *max_radius = 0;
  for (int r = 0; r < R; ++r) {
    const long long op = rules[3 * r], n = rules[3 * r + 1], to = rules[3 * r + 2];
    EFFQ_CHECK_ARG(op >= EFFQ_LABEL_CLEAN_LARGEST && op <= last_op);
    EFFQ_CHECK_ARG(op != EFFQ_LABEL_CLEAN_MIN || n >= 1);
    const bool ball = op == EFFQ_LABEL_POST_CLOSE || op == EFFQ_LABEL_POST_OPEN;
    EFFQ_CHECK_ARG(!ball || (n >= 1 && n <= EFFQ_LABEL_POST_MAX_RADIUS));
    EFFQ_CHECK_ARG(to >= 0 && to <= 255);
    // fill and close add voxels to the mask: TO is one of its values; the other ops take voxels out of it
    const bool grows = op == EFFQ_LABEL_POST_FILL || op == EFFQ_LABEL_POST_CLOSE;
    EFFQ_CHECK_ARG(sets[256 * r] == 0 && (sets[256 * r + to] != 0) == grows);
    if (ball && n > *max_radius) *max_radius = (int)n;
    for (int k = 0; k < 4; ++k) set[r].w[k] = 0ull;
    for (int v = 0; v < 256; ++v)
      if (sets[256 * r + v]) set[r].w[v >> 6] |= 1ull << (v & 63);
  }
  return EFFQ_OK;
}

}  // namespace effq
using namespace effq;

extern "C" {

size_t effq_label_clean_ws_bytes(int D, int H, int W) {
  if (!cc_dims_ok(1, D, H, W)) return 0;
  return clean_ws(nullptr, (size_t)D * H * W).bytes;
}

int effq_label_clean(const uint8_t* in, int D, int H, int W, int connectivity, int R, const uint8_t* sets,
                     const long long* rules, uint8_t* out, long long* stats, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(in && sets && rules && out && stats && ws);
  EFFQ_CHECK_ARG(R >= 1 && R <= EFFQ_LABEL_CLEAN_MAX_RULES);
  EFFQ_CHECK_ARG(cc_dims_ok(1, D, H, W));
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  CleanSet set[EFFQ_LABEL_CLEAN_MAX_RULES];
  int max_radius;
  int rc = post_parse_rules(R, sets, rules, EFFQ_LABEL_CLEAN_MIN, set, &max_radius);
  if (rc != EFFQ_OK) return rc;
  const int S = D * H * W;
  const CleanWs s = clean_ws(ws, (size_t)S);
  EFFQ_CHECK_WS(ws_bytes, s.bytes);
  const hipStream_t st = as_stream(stream);
  if (out != in) EFFQ_HIP(hipMemcpyAsync(out, in, (size_t)S, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_clean_init, dim3(1), dim3(64), 0, st, s.best, stats, R);
  EFFQ_LAUNCH_CHECK();
  for (int r = 0; r < R; ++r) {
    rc = clean_rule_run(s, set[r], rules + 3 * r, D, H, W, connectivity, out, stats + 2 * r, s.best + r, st);
    if (rc != EFFQ_OK) return rc;
  }
  return EFFQ_OK;
}

size_t effq_label_post_ws_bytes(int D, int H, int W, int max_radius) {
  if (!post_dims_ok(D, H, W, max_radius)) return 0;
  return post_ws(nullptr, D, H, W, max_radius).bytes;
}

int effq_label_post(const uint8_t* in, int D, int H, int W, int connectivity, int R, const uint8_t* sets,
                    const long long* rules, uint8_t* out, long long* stats, void* ws, size_t ws_bytes, void* stream) {
  EFFQ_CHECK_ARG(in && sets && rules && out && stats && ws);
  EFFQ_CHECK_ARG(R >= 1 && R <= EFFQ_LABEL_CLEAN_MAX_RULES);
  EFFQ_CHECK_ARG(connectivity == 6 || connectivity == 26);
  CleanSet set[EFFQ_LABEL_CLEAN_MAX_RULES];
  int max_radius;
  int rc = post_parse_rules(R, sets, rules, EFFQ_LABEL_POST_OPEN, set, &max_radius);
  if (rc != EFFQ_OK) return rc;
  EFFQ_CHECK_ARG(post_dims_ok(D, H, W, max_radius));
  const int S = D * H * W;
  const PostWs s = post_ws(ws, D, H, W, max_radius);
  EFFQ_CHECK_WS(ws_bytes, s.bytes);
  const hipStream_t st = as_stream(stream);
  if (out != in) EFFQ_HIP(hipMemcpyAsync(out, in, (size_t)S, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_clean_init, dim3(1), dim3(64), 0, st, s.clean.best, stats, R);
  EFFQ_LAUNCH_CHECK();
  for (int r = 0; r < R; ++r) {
    const long long op = rules[3 * r];
    const int n = (int)rules[3 * r + 1], to = (int)rules[3 * r + 2];
    if (op == EFFQ_LABEL_POST_FILL)
      rc = post_fill_run(s, set[r], to, D, H, W, connectivity == 26 ? 6 : 26, out, stats + 2 * r, st);
    else if (op == EFFQ_LABEL_POST_CLOSE)
      rc = post_ball_run<false>(s, set[r], n, to, D, H, W, out, stats + 2 * r, st);
    else if (op == EFFQ_LABEL_POST_OPEN)
      rc = post_ball_run<true>(s, set[r], n, to, D, H, W, out, stats + 2 * r, st);
    else
      rc = clean_rule_run(s.clean, set[r], rules + 3 * r, D, H, W, connectivity, out, stats + 2 * r, s.clean.best + r, st);
    if (rc != EFFQ_OK) return rc;
  }
  return EFFQ_OK;
}

}  // extern "C"
