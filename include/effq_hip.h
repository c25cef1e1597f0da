/*
 * effq_hip.h -- C ABI of the MI355X (gfx950) hot path of EfficientQ's layer-wise
 * PTQ calibration.  This is the drop-in boundary: plain pointers and sizes, no
 * torch types, every call returns an int status (EFFQ_OK == 0; no exceptions
 * cross the ABI), every buffer is a caller-owned DEVICE pointer unless the
 * parameter says "host", every call takes the HIP stream to enqueue on
 * (a hipStream_t passed as void*; NULL = default stream) and never
 * synchronises unless documented.  The reference has no FFI of its own (it is
 * pure Python); each entry point cites the reference code it
 * replaces (paths relative to the reference checkout).
 *
 * Layouts
 *   activations / targets : NDHWC fp32 (torch channels_last_3d), x[n][d][h][w][c]
 *   attention mask        : [n][D'][H'][W'] fp32 (one weight per output voxel)
 *   weights               : reference layout [c2][c1][kd][kh][kw] fp32
 *   Gram system           : A0 [n x n], B0 [c2 x n] row-major fp32, n = c1*k^3 (+1 bias),
 *                           row order (c1,kd,kh,kw)+bias exactly as solver.py:104-108,256
 */
#ifndef EFFQ_HIP_H
#define EFFQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  EFFQ_OK = 0,
  EFFQ_ERR_ARG = 1,        /* bad argument (null pointer, bad shape, unsupported geometry) */
  EFFQ_ERR_HIP = 2,        /* a HIP runtime call failed; see effq_last_error() */
  EFFQ_ERR_WORKSPACE = 3,  /* workspace too small; query the *_ws_bytes function */
  EFFQ_ERR_NO_DEVICE = 4,
  EFFQ_ERR_NOT_CONVERGED = 5
};

/* Conv geometry.  Dilation and groups are 1 (the reference's solver ignores
 * them, solver.py:86-111, and both shipped configs use 1). */
typedef struct effq_geom {
  int32_t N, C1, C2;
  int32_t D, H, W;          /* input spatial size  */
  int32_t KD, KH, KW;       /* 1 or 3 per axis      */
  int32_t SD, SH, SW;       /* stride               */
  int32_t PD, PH, PW;       /* symmetric zero pad   */
} effq_geom;

const char* effq_last_error(void);
int effq_version(void);
/* Number of HIP devices visible; does not initialise a context. */
int effq_device_count(int* count);

/* ---- a1/a3: discretize + PTQConv._quantize_act -------------------------------
 * layer_helper.py:25-37, PTQConv.py:114-116.
 * fp32 path: y = (rint((clamp(x/alpha,lo,hi)-lo)/d)*d+lo)*alpha with d=f32((hi-lo)/(L-1)),
 * IEEE divisions, round-half-even, no FMA contraction.  alpha is read from DEVICE
 * memory (one float).  idx_out (uint8 level ids) and y_out may each be NULL.
 * Non-finite inputs follow torch: -inf / +inf land on level 0 / L-1, a NaN stays NaN in y_out
 * (torch.clamp propagates it); the level id written for a NaN is unspecified. */
int effq_quant_dequant_f32(const float* x, const float* alpha_dev, float lo, float hi, int levels,
                           float* y_out, uint8_t* idx_out, size_t n, void* stream);

/* fp64 path used during calibration (project_by_iter's final discretize,
 * layer_helper.py:50-66, then "a * b", EfficientQConv.py:68-70):
 * b = f32(discretize(f64(x)/alpha)), y = f32(alpha)*b.  alpha is a DEVICE double.
 * y_out, b_out and idx_out may each be NULL.  A NaN in x is NaN in b_out and y_out; its level
 * id is unspecified, as above. */
int effq_quant_dequant_f64path(const float* x, const double* alpha_dev, double lo, double hi, int levels,
                               float* y_out, float* b_out, uint8_t* idx_out, size_t n, void* stream);

/* ---- a2: project_by_iter pieces (layer_helper.py:40-70) -----------------------
 * Workspace for all reductions below: effq_reduce_ws_bytes() bytes, zero-initialised
 * once by the caller (hipMemset) and then owned by this library between calls. */
size_t effq_reduce_ws_bytes(void);

/* sums_out[0] = sum |x_i| (fp64), sums_out[1] = n (2 doubles).  (a = var.abs().mean(), layer_helper.py:51) */
int effq_abs_sum_f64(const float* x, size_t n, double* sums_out, void* ws, void* stream);

/* sums_out[0] = sum x, [1] = sum x^2 (fp64), [2] = n.  (Tensor.std(), EfficientQConv.py:46,48) */
int effq_moments_f64(const float* x, size_t n, double* sums_out, void* ws, void* stream);

/* One fixed-point statistics pass: b = discretize(f64(x)/alpha); sums_out[0] = sum b*x,
 * sums_out[1] = sum b*b (layer_helper.py:57-59).  alpha is a DEVICE double.  If
 * done_flag_dev is non-NULL and *done_flag_dev != 0 the pass is skipped. */
int effq_alpha_stats_f64(const float* x, const double* alpha_dev, double lo, double hi, int levels,
                         size_t n, double* sums_out, const int32_t* done_flag_dev, void* ws, void* stream);

/* Fixed-point state on the device: {alpha, alpha_prev, sums[2], iters, done}. */
typedef struct effq_fp_state {
  double alpha;
  double alpha_prev;
  double sums[2];
  int32_t iters;
  int32_t done;      /* 1 converged, 2 hit max_iter (the reference raises, layer_helper.py:62-64) */
} effq_fp_state;

/* state.alpha = sums[0]/sums[1] (abs-mean start), alpha_prev=-999, iters=0, done=0. */
int effq_fp_init(effq_fp_state* state_dev, const double* abs_sums_dev, void* stream);
/* alpha_prev=alpha; alpha=sums[0]/sums[1]; ++iters; done when |alpha-alpha_prev|<=tol or iters==max_iter.
 * Reads state->sums (so an all-reduce of state->sums may run between stats and update). */
int effq_fp_update(effq_fp_state* state_dev, double tol, int max_iter, void* stream);

/* Fixed point on the stream without host round trips: runs `n_iters` fused iterations (statistics pass
 * whose last block also applies the update; each a no-op once done).  The caller checks state.done. */
int effq_alpha_fixed_point(const float* x, size_t n, int levels, double lo, double hi, double tol,
                           int max_iter, int n_iters, effq_fp_state* state_dev, void* ws, void* stream);

/* Whole project_by_iter of a SMALL tensor (n <= effq_fp_small_max()) in one launch, no host round trip:
 * v = a + b (b may be NULL; v is written to v_out when given, required if b != NULL), alpha0 = mean|v|,
 * then the fixed point runs on chip until |d alpha| <= tol or max_iter.  The ADMM weight projection of
 * most layers (EfficientQConv.py:108 -> layer_helper.py:40-70). */
size_t effq_fp_small_max(void);
int effq_fixed_point_small(const float* a, const float* b, float* v_out, size_t n, int levels, double lo, double hi,
                           double tol, int max_iter, effq_fp_state* state_dev, void* stream);
/* Same contract for larger tensors (n <= effq_fp_coop_max()): one COOPERATIVE launch of ceil(n/27648) <= 256
 * workgroups (one per CU, slice of v resident in LDS) that meet at a bounded-spin grid barrier once per
 * iteration; partial sums are combined in workgroup order by every workgroup (deterministic).  state.done = 3
 * reports a barrier time-out.  ws: the reduction workspace (effq_reduce_ws_bytes()), zero-filled once by the caller:
 * the kernel keeps its barrier words in the tail of it and leaves them at zero.  A time-out POISONS the workspace: every
 * later launch on it (e.g. the following ADMM iterations, already enqueued) returns at once with state.done = 3 and
 * touches nothing, until the caller zero-fills the workspace again.
 * effq_fp_coop_set_spin_limit: polls a workgroup waits at the barrier before it gives up (0 = the default, 2^24); a
 * process-wide test hook - tests force the time-out path with a small value. */
size_t effq_fp_coop_max(void);
int effq_fixed_point_coop(const float* a, const float* b, float* v_out, size_t n, int levels, double lo, double hi,
                          double tol, int max_iter, effq_fp_state* state_dev, void* ws, void* stream);
int effq_fp_coop_set_spin_limit(unsigned int polls);
/* Same contract again (n <= effq_fp_bucket_max(), levels <= 256) without a per-iteration pass over the tensor: the
 * values are counted into equal-width buckets (exact integer sum per bucket) and regrouped by bucket once; each
 * iteration then reads prefix tables and looks only at the values of the bucket a level boundary falls into (those in
 * a 1e-6 relative guard band around the boundary are classified with the reference's own fp64 arithmetic).  Level
 * counts are exactly the reference's, alpha agrees to ~1e-14 relative (fp64 sums in another order), same iteration
 * count; deterministic (integer partial sums).  n <= 32768: one workgroup, everything in LDS, ws unused.  Larger:
 * four launches (sum|v| and range / count with global atomics / scan / regroup + iterate in the last workgroup to
 * finish).  ws: effq_fp_bucket_ws_bytes(n) bytes, ZERO-FILLED once by the caller and owned by the library between
 * calls (its counters are left at zero). */
size_t effq_fp_bucket_max(void);
size_t effq_fp_bucket_ws_bytes(size_t n);
int effq_fixed_point_bucket(const float* a, const float* b, float* v_out, size_t n, int levels, double lo, double hi,
                            double tol, int max_iter, effq_fp_state* state_dev, void* ws, size_t ws_bytes,
                            void* stream);

/* project_by_iter for the weight projection INSIDE the ADMM loop (EfficientQConv.py:108 -> layer_helper.py:40-70) in ONE
 * launch, from the previous ADMM iteration's iterates: v_k = w*_k + dual_{k-1} differs little from v_{k-1}, so the i-th
 * iterate of this call lies within 1e-3 ... 1e-9 of the i-th iterate of the last one.  `pred_dev`
 * (effq_fp_traj_pred_bytes() bytes of device memory, zero-filled = nothing known) carries them from call to call with a
 * margin each.  One pass over the values by all workgroups forms v, sums |v| and tallies - in integers - every value
 * whose level is the same at both ends of a predicted bracket (the level is monotone in the scale); the few per cent
 * that are not go to a list.  The last workgroup to finish then iterates: an iterate inside its predicted bracket costs
 * one scan of the list; one outside costs a pass of that single workgroup over v (slow, rare).  Levels are exactly the
 * reference's, alpha within ~1e-15 of the fp64 kernels', same iteration count, deterministic.  levels <= 16,
 * n <= effq_fp_traj_max().  ws: effq_fp_traj_ws_bytes(n), zero-filled once (its counters are left at zero).
 * The *_rec variants of the older fixed points do the same work as their namesakes and, when pred_dev != NULL, leave
 * their iterates in it (the first call of a layer, calls after rho has changed). */
size_t effq_fp_traj_max(void);
size_t effq_fp_traj_ws_bytes(size_t n);
size_t effq_fp_traj_pred_bytes(void);
int effq_fixed_point_traj(const float* a, const float* b, float* v_out, size_t n, int levels, double lo, double hi,
                          double tol, int max_iter, effq_fp_state* state_dev, void* pred_dev, void* ws, size_t ws_bytes,
                          void* stream);
int effq_fixed_point_bucket_rec(const float* a, const float* b, float* v_out, size_t n, int levels, double lo, double hi,
                                double tol, int max_iter, effq_fp_state* state_dev, void* ws, size_t ws_bytes,
                                void* pred_dev, void* stream);
int effq_fixed_point_coop_rec(const float* a, const float* b, float* v_out, size_t n, int levels, double lo, double hi,
                              double tol, int max_iter, effq_fp_state* state_dev, void* ws, void* pred_dev, void* stream);

/* project_by_iter (layer_helper.py:40-70) on tensors far too large for the chip - the activations of a layer
 * (PTQConv.py:74-78, EfficientQConv.py:64-72) - without a pass over the whole tensor per iteration.  The level of a value
 * is monotone in the scale, so a value whose level is the same at both ends of a bracket that confines the remaining
 * iterates is settled: a narrowing pass moves its contribution into integer tallies and leaves the unsettled values in
 * a compact list, which is all the following iterations read (and narrow further).  The bracket is a prediction from
 * the last iterates (up to the limit of the sequence, or a horizon of a few iterations while it converges slowly); an
 * iterate that leaves it restarts from the tensor or the list of its non-zeros (correctness never depends on it).
 * Levels are exactly the reference's in every iteration; sums are integers in units of 2^-e (order-independent:
 * deterministic, identical for any split of the tensor); alpha agrees with the fp64 kernels to ~1e-13, same iteration
 * count.  levels <= 256.
 *   init  : state.alpha = abs_sums[0] / abs_sums[1] (the all-reduced sum|x| and count: abs-mean start), unit and plan;
 *           list_first != 0: the first pass already lists the values that are not settled for every scale (the
 *           non-zeros - worth it for post-ReLU tensors, a wasted copy for dense ones).
 *   run   : n_iters x {iteration pass + finish (sums, scalar update, plan of the next pass)}; no-ops once state.done.
 *   stats : one iteration pass, state.sums = this rank's [sum b*x, sum b*b]   } with data-parallel ranks the caller
 *   update: scalar update from state.sums + plan of the next pass              } all-reduces state.sums in between
 * ws: effq_fp_bracket_ws_bytes(n) bytes (three lists of n floats + tallies), owned by the fit between init and its end.
 * The first 256 bytes of ws are the fit's header as 8-byte words (FbrHdr of fixed_point_bracket.hip): the first sixteen
 * are diagnostics (bracket, plan, escapes, narrowings, values read), the planning and import state follows; the tests
 * read all of them by word index. */
size_t effq_fp_bracket_ws_bytes(size_t n);
int effq_fp_bracket_init(effq_fp_state* state_dev, const double* abs_sums_dev, size_t n, int levels, int list_first,
                         void* ws, size_t ws_bytes, void* stream);
int effq_fp_bracket_run(const float* x, size_t n, int levels, double lo, double hi, double tol, int max_iter, int n_iters,
                        effq_fp_state* state_dev, void* ws, void* stream);
int effq_fp_bracket_stats(const float* x, size_t n, int levels, double lo, double hi, effq_fp_state* state_dev, void* ws,
                          void* stream);
int effq_fp_bracket_update(size_t n, int levels, double lo, double hi, double tol, int max_iter,
                           effq_fp_state* state_dev, void* ws, void* stream);
/* Data-parallel ranks, "gather once": after a few all-reduced iterations (stats / update above) a rank's shard is, under
 * the current bracket, four integer tallies of the decided values + the list of the undecided ones.
 *   export: out (effq_fp_bracket_export_words() int64): [0..3] = the tallies, [4] = the list's length (-1: no list yet, -2:
 *           the current bracket is a horizon the iterates are meant to leave - many levels - so not worth exchanging),
 *           [5], [6] = the bit patterns of the bracket [blo, bhi] the tallies and the list are valid under (ranks plan on
 *           their own shard: brackets may differ), the rest scratch; list_out[0 .. list_cap) = the list, zero-filled behind
 *           it (all zeros if there is none or it does not fit).  The caller all-reduces a pack {tallies[4], then per rank
 *           (length, blo bits, bhi bits)} and all-gathers the list_cap floats of every rank (zero padding is harmless for
 *           the unsigned quantiser lo = 0: an exact zero has level 0 at every scale);
 *   import: sets up ws_dst (effq_fp_bracket_ws_bytes(world * list_cap)) as a fit over the gathered lists with the summed
 *           tallies as its constant part and the iterates / unit of ws_src, valid under the INTERSECTION of the ranks'
 *           brackets; effq_fp_bracket_run(gathered, world * list_cap, ..., ws_dst) then finishes WITHOUT collectives,
 *           bit-identically on every rank.  Whether the exchange is usable (every list fitted, the iterate lies in the
 *           intersection) is decided on the device - the host never needs the lengths: if not, or once an iterate leaves
 *           that bracket, state.done = 4 (the launches that follow are no-ops) and the caller goes on with stats / update
 *           on the rank's own workspace after effq_fp_bracket_rebase. */
size_t effq_fp_bracket_export_words(void);
int effq_fp_bracket_export(const void* ws, size_t n, long long* out, float* list_out, size_t list_cap, void* stream);
int effq_fp_bracket_import(const void* ws_src, size_t n_src, const long long* pack_dev, int world, size_t list_cap,
                           effq_fp_state* state_dev, void* ws_dst, size_t ws_dst_bytes, void* stream);
/* after state.done = 4: clears it and makes the rank's OWN workspace start its next pass from the base (its list and
 * tallies belong to a bracket the iterates have moved on from while the imported fit ran) */
int effq_fp_bracket_rebase(effq_fp_state* state_dev, void* ws, size_t n, void* stream);
/* Per-output-channel scales (fixed_point_channels.hip): project_by_iter on every row of v = a + b ([c2][nwrow], b may be
 * NULL; v is written to v_out when given, required if b != NULL) on its own, weight grid lo = -1, hi = 1: a0 = mean|v_c|,
 * then the fixed point until |d alpha| <= tol or max_iter.  alpha_out[c2] (fp64), iters_out[c2] (may be NULL),
 * *err_flag_dev = 2 (sticky; may be NULL) when a row hit max_iter.  A row with sum|v_c| = 0 gets alpha 0, 0 iterations,
 * converged.  One workgroup per row, no grid barrier; deterministic.  nwrow <= effq_fp_channels_max_row().
 * _proj: with a = wstar, b = dual, the ADMM projection + dual update of every row in the same launch: G = alpha_c b
 * (0 on a zero row), dual <- (wstar - G + dual) / dual_div, and, with Bm != NULL, the next prox right-hand side
 * Bm[r][k] = (B0[r][k] + eta W0) + rho_next (G - dual) (rows of B0 n long, of Bm ldb long), as effq_project_dual_next. */
int effq_fp_channels_max_row(void);
int effq_fixed_point_channels(const float* a, const float* b, float* v_out, int c2, int nwrow, int levels, double tol,
                              int max_iter, double* alpha_out, int32_t* iters_out, int32_t* err_flag_dev, void* stream);
int effq_fixed_point_channels_proj(const float* wstar, float* dual, float* v_out, int c2, int nwrow, int levels,
                                   double tol, int max_iter, double* alpha_out, int32_t* iters_out, int32_t* err_flag_dev,
                                   float* G, float dual_div, float* Bm, const float* B0, const float* W0, int n, int ldb,
                                   double rho_next, double eta, void* stream);

/* Sticky device-side check used by stream-resident loops: *err_flag_dev = 2 (cap hit; the reference
 * raises, layer_helper.py:62-64) or 3 (not finished) unless state.done == 1. */
int effq_fp_check(const effq_fp_state* state_dev, int32_t* err_flag_dev, void* stream);

/* ---- a5/a6: im2col + getA0B0 (solver.py:86-111, 282-314), never materialising x_col ----
 * A0 = 2*sum_v att_v xhat_v xhat_v^T, B0 = 2*sum_v att_v y_v xhat_v^T; xhat has a trailing 1
 * when has_bias.  att may be NULL (all ones).  accumulate!=0 adds into A0/B0 (sharded volumes).
 * ws: effq_gram_ws_bytes(geom) bytes. */
size_t effq_gram_ws_bytes(const effq_geom* g, int has_bias);
int effq_gram_accum(const float* x_ndhwc, const float* att, const float* y_ndhwc, const effq_geom* g,
                    int has_bias, float* A0, float* B0, int accumulate, void* ws, size_t ws_bytes,
                    void* stream);
/* The launch effq_gram_accum makes for a geometry; launches nothing.  *vec: 1 = the kernel that stages 16-byte cells
 * (C1 and C2 multiples of 4), 0 = the row-by-row kernel; the grid is *npairs blocks of the upper block triangle (*nb
 * 128-row blocks per side) x *nsplit voxel ranges of *vox_per_split voxels; the fp32 accumulators are folded into fp64 every
 * *fold chunks of 32 voxels; *finish_blocks groups of 256 threads (four workgroups each) add the slabs up (8192 at most, strided beyond). */
int effq_gram_plan_query(const effq_geom* g, int has_bias, int* vec, int* nb, int* npairs, int* nsplit,
                         long long* vox_per_split, int* fold, int* finish_blocks);
/* 1 where effq_gram_accum gathers these inputs with the streamed kernel (C1 a multiple of 4 and x 16-byte aligned; y by
 * 16-byte cells where C2 is a multiple of 4 and y is aligned, by values up to C2 = 32 otherwise), 0 where with the kernels
 * *vec of effq_gram_plan_query names; both give the same bits.  Launches nothing. */
int effq_gram_streamed(const float* x_ndhwc, const float* y_ndhwc, const effq_geom* g, int has_bias);
/* The second launch of effq_gram_accum alone (profiling): A0 / B0 from the slabs a previous effq_gram_accum of the same
 * geometry left in ws. */
int effq_gram_finish(const effq_geom* g, int has_bias, float* A0, float* B0, int accumulate, void* ws, size_t ws_bytes,
                     void* stream);

/* The same A0/B0 for a layer whose input is already quantised (EfficientQConv.py:64-72 ran first), evaluated
 * exactly on the i8 matrix cores: xidx = level ids of the quantised input (uint8, NDHWC, value k means
 * xhat = alpha_act*k/(act_levels-1)), act_alpha_dev = device float.  The attention weights enter as a voxel
 * list sorted by weight value: vox_list[n_list] (output-voxel indices, -1 = padding; every run of 128 entries
 * has one weight), chunk_cls[n_list/128] = class of each run, cls_w_dev[ncls] = the class weights (device
 * floats, ncls <= 16).  vox_list == NULL: all weights 1 (then chunk_cls = NULL, ncls = 1, n_list = 0).
 * Requires effq_gram_i8_supported (C1 % 16 == 0, at most 31 taps, act_levels <= 128); results equal
 * effq_gram_accum on xhat up to the fp32 rounding of that path (integer sums here are exact).
 * ws: effq_gram_i8_ws_bytes(geom, ncls). */
int effq_gram_i8_supported(const effq_geom* g, int act_levels);
size_t effq_gram_i8_ws_bytes(const effq_geom* g, int ncls);
int effq_gram_accum_i8(const uint8_t* xidx_ndhwc, const float* y_ndhwc, const effq_geom* g, int has_bias,
                       const float* act_alpha_dev, int act_levels, const int32_t* vox_list,
                       const int32_t* chunk_cls, const float* cls_w_dev, int ncls, long long n_list,
                       float* A0, float* B0, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* The same pass with the UNWEIGHTED system as a by-product, in fp64: Au [n][n] = sum_v xhat xhat^T (reference row order,
 * ones row included, no factor 2), Bu [c2][n] = sum_v y xhat^T - the integer class slabs summed without the attention
 * weights.  Au / Bu may both be NULL (= effq_gram_accum_i8). */
int effq_gram_accum_i8_unw(const uint8_t* xidx_ndhwc, const float* y_ndhwc, const effq_geom* g, int has_bias,
                           const float* act_alpha_dev, int act_levels, const int32_t* vox_list, const int32_t* chunk_cls,
                           const float* cls_w_dev, int ncls, long long n_list, float* A0, float* B0, int accumulate,
                           double* Au, double* Bu, void* ws, size_t ws_bytes, void* stream);
/* The launch effq_gram_accum_i8* makes for a geometry and a voxel list of n_list slots (0: no list); launches nothing.
 * *nb 128-row blocks per side of the extended integer system, the first *nbx of them hold x rows, *npairs block pairs x
 * *nsplit splits of *cps chunks (128 voxels each, *nchunks in all); a split accumulates in int32 and flushes per class. */
int effq_gram_i8_plan_query(const effq_geom* g, int ncls, long long n_list, int* nb, int* nbx, int* npairs, int* nchunks,
                            int* cps, int* nsplit);
/* Which of those block pairs one workgroup computes; launches nothing.  A workgroup owns *gi x *gj adjacent blocks and
 * stages their rows once per chunk for all of its pairs: the grid is *ngroups x *grid_y.  2 x 2 on systems with at least
 * two block rows (nbx >= 2) whose splits hold at least 64 chunks, and there every split is cut into two workgroups
 * (*grid_y = 2 nsplit); 1 x 1 otherwise (one pair per workgroup, *ngroups = npairs, *grid_y = nsplit).  The plan above,
 * the slabs and with them every output bit do not depend on the grouping.
 * effq_gram_i8_set_group: process-wide override of that rule (test hook): (1, 1) one pair per workgroup everywhere (the
 * launch without groups), (2, 2) groups everywhere (splits still cut in two only from 64 chunks on); (0, 0) restores the
 * rule.  Anything else: EFFQ_ERR_ARG. */
int effq_gram_i8_group_query(const effq_geom* g, int ncls, long long n_list, int* gi, int* gj, int* ngroups, int* grid_y);
int effq_gram_i8_set_group(int gi, int gj);

/* The unweighted system of a layer whose input is NOT quantised (first conv / classifier, q_first = q_last = "256,-1":
 * definer.py:296-299, model_blk.py:98-107), in fp64 on the matrix cores: Au [n][n] = sum_v xhat xhat^T with
 * xhat = [im2col patch of x (solver.py:86-111 row order); 1 if has_bias], Bu [c2][n] = sum_v y xhat^T.  fp32 inputs, exact
 * products, fp64 accumulation, deterministic (partial slabs added in workgroup order).  Operands of effq_gram_loss for
 * those layers.  Requires effq_gram_f64_supported (n = C1*KD*KH*KW + has_bias <= 128, C2 <= 64).
 * ws: effq_gram_f64_ws_bytes(geom, has_bias). */
int effq_gram_f64_supported(const effq_geom* g, int has_bias);
size_t effq_gram_f64_ws_bytes(const effq_geom* g, int has_bias);
int effq_gram_f64(const float* x_ndhwc, const float* y_ndhwc, const effq_geom* g, int has_bias, double* Au, double* Bu,
                  void* ws, size_t ws_bytes, void* stream);
/* The launch effq_gram_f64 makes for a supported geometry; launches nothing.  *grid persistent workgroups (1024 at most)
 * walk *nchunk chunks of 32 voxels; *ntiles 16 x 16 accumulator tiles, *tpw (3, 6, 11 or 18) of them per wave. */
int effq_gram_f64_plan_query(const effq_geom* g, int has_bias, int* nchunk, int* grid, int* ntiles, int* tpw);
/* 1 where effq_gram_f64 gathers these inputs with its pipelined loop (C1 % 4 == 0, x 16-byte aligned, at most four 16-byte
 * cells of x and one cell - C2 % 4 == 0 and y 16-byte aligned - or value of y per thread and 32-voxel chunk, at most 11 tiles
 * per wave), 0 where with the plain loop or for an unsupported geometry.  Both loops stage the same values: the results
 * do not depend on the answer.  Launches nothing. */
int effq_gram_f64_pipelined(const float* x_ndhwc, const float* y_ndhwc, const effq_geom* g, int has_bias);

/* ---- the loss of one iterate from the unweighted Gram system (EfficientQConv.py:118-122 without the pass over the voxels)
 * sum_v,c (conv(Qx, G, b)_v,c - y_v,c)^2 = sum_c g_c^T Au g_c - 2 sum_c g_c . Bu_c + syy with g_c = [G[c,:], b_c], in fp64:
 * sqerr_out[0] = sqerr_out[1] = that sum (the unweighted squared error, as the conv entry points report it).  c2 n^2
 * multiply-adds on an n x n matrix instead of a pass over all voxels: for layers whose voxel count is far above n.
 * ws: effq_gram_loss_ws_bytes(n), zero-filled once by the caller. */
size_t effq_gram_loss_ws_bytes(int n);
int effq_gram_loss(const double* Au, const double* Bu, const double* syy_dev, const float* G, const float* b, int c2, int n,
                   int has_bias, double* sqerr_out, void* ws, size_t ws_bytes, void* stream);

/* ---- the same losses for a GROUP of iterates of a wide layer, the quadratic form on the i8 matrix cores (exact integers)
 * sum_c w_c^T Aww w_c = s_w^2 s_a^2 <K, J^T J> with K = Aww / s_a^2 (integer: sums of products of level ids) and
 * J = the int8 level numerators of the iterate (Gq ring of effq_admm_run, as for conv3d_calib_step_i8).
 *   effq_gram_loss_i8_supported: c2 % 32 == 0, (n - has_bias) % 64 == 0, w_levels <= 64;
 *   effq_gram_loss_i8_num_planes(kmax): balanced base-256 digit planes for entries up to kmax (<= (La-1)^2 * voxels), -1 if > 6;
 *     P planes of digits -128 .. 127 hold 0 .. 127 (256^P - 1) / 255 (127, 32639, 8355711, ...);
 *   effq_gram_loss_i8_prepare: planes [P][round_up(n - has_bias, 256)][n - has_bias] int8 from Au (effq_gram_accum_i8_unw),
 *     once per layer; *err_flag_dev is set non-zero if Au is not the integer system it should be;
 *   effq_gram_loss_i8: hist_out[j][0] = hist_out[j][1] = sum (out - y)^2 of iterate j = 0 .. count-1 (count <= 16):
 *     Gq [count][c2][n - has_bias], b [count][c2] (NULL without bias), states[j].alpha = the iterate's weight scale;
 *     out = f32(alpha_a) f32(alpha_w) / ((La-1)(Lw-1)) * (J . k) + b in exact arithmetic (the contract of
 *     conv3d_calib_step_i8), evaluated in integers and fp64.  ws: effq_gram_loss_i8_ws_bytes(), zero-filled once. */
int effq_gram_loss_i8_supported(int c2, int n, int has_bias, int w_levels);
int effq_gram_loss_i8_num_planes(long long kmax);
size_t effq_gram_loss_i8_planes_bytes(int n, int has_bias, int nplanes);
int effq_gram_loss_i8_prepare(const double* Au, int n, int has_bias, const float* act_alpha_dev, int act_levels,
                              int nplanes, int8_t* planes, int32_t* err_flag_dev, void* stream);
size_t effq_gram_loss_i8_ws_bytes(void);
int effq_gram_loss_i8(const int8_t* planes, int nplanes, const double* Au, const double* Bu, const double* syy_dev,
                      const int8_t* Gq, const float* b, const effq_fp_state* states, const float* act_alpha_dev,
                      int act_levels, int w_levels, int c2, int n, int has_bias, int count, double* hist_out, void* ws,
                      size_t ws_bytes, void* stream);


/* The voxel list of an attention mask, by three small kernels (distinct weights + counts, segment layout, scatter): the
 * class weights are the few integers quirk Q1 leaves (ptqer.py:161-165).  vox_list: V + 2048 int32, chunk_cls: V/128 + 16
 * int32, cls_w_dev: 16 floats, ws: effq_att_classes_ws_bytes().  info_host_out[3] = {ncls, n_list, overflow}; the call
 * synchronises the stream to return them (once per mask; the layers of a pyramid level share it).  overflow != 0: more
 * than 16 distinct weights (use effq_gram_accum).  The order of the voxels inside a class is not fixed; the sums of
 * effq_gram_accum_i8 are exact integers, so its results do not depend on it. */
size_t effq_att_classes_ws_bytes(void);
int effq_att_classes(const float* att, long long V, int32_t* vox_list, int32_t* chunk_cls, float* cls_w_dev,
                     int32_t* info_host_out, void* ws, void* stream);

/* Creates the helper stream the 256-row sweep keeps per caller stream (otherwise created by the first large inverse): call it
 * for every stream inverses will run on BEFORE anything else creates streams (a communicator, a framework pool), so that the
 * calibration's streams keep hardware queues of their own. */
int effq_spd_inverse_prepare(void* stream);
/* ---- a7: getAB + solve (solver.py:316-345) --------------------------------------
 * Ainv = (A0 + rho*I' + eta*I)^-1 in fp64 (I' has 0 on the bias diagonal), stored fp32 as n rows of
 * effq_ainv_ld(n) floats (row padding is zero; exactly symmetric).
 * The reference refactorises per iteration; A only changes with rho (5 values per layer). */
int effq_ainv_ld(int n);
size_t effq_spd_inverse_ws_bytes(int n);
int effq_spd_inverse(const float* A0, int n, int has_bias, double rho, double eta, float* Ainv,
                     void* ws, size_t ws_bytes, void* stream);
/* Which sweep effq_spd_inverse runs for a system of n rows; launches nothing.  *wide: 1 = the sweep with 256-row pivot
 * blocks, 0 = the rank-64 sweep; *nblk: 64-blocks per side of the padded matrix; *pivot_blocks: elimination steps (the last
 * pivot block of a wide sweep holds the remaining 1 .. 4 64-blocks). */
int effq_spd_inverse_plan(int n, int* wide, int* nblk, int* pivot_blocks);

/* What = (B0 + eta*[W0|b0] + rho*[G-dual|0]) * Ainv ; splits into wstar [c2 x (n-1|n)] and bstar [c2].
 * W0, G, dual, wstar in reference weight layout (contiguous c2 x c1k).  b0/bstar NULL when !has_bias.
 * rho/eta are host doubles.  ws: effq_prox_ws_bytes(c2,n). */
size_t effq_prox_ws_bytes(int c2, int n);
int effq_prox_solve(const float* B0, const float* Ainv, const float* W0, const float* b0, const float* G,
                    const float* dual, int c2, int n, int has_bias, double rho, double eta, float* wstar,
                    float* bstar, void* ws, size_t ws_bytes, void* stream);
/* The GEMM the prox solves of a c2 x n system run; launches nothing.  *variant: 0 - 3 = the f32 matrix-core kernel with
 * 256 / 128 / 64 / 32 rows per workgroup, 5 / 7 = the bf16x3 kernel with 256 / 128 rows; the grid is gx column tiles x gy
 * row tiles x nsplit K slices (nsplit > 1: partial products, added up in slice order). */
int effq_prox_plan_query(int c2, int n, int* variant, int* gx, int* gy, int* nsplit);

/* The same solve for A(rho) when only Ainv = A(rho_inv)^-1 is at hand (rho_inv >= rho): A(rho) = A(rho_inv) -
 * d*I' with d = rho_inv - rho, so What = (B + d*[What_w|0]) * Ainv is a contraction with factor
 * < d/(rho_inv + eta) (1/2 for the reference's doubling schedule, EfficientQConv.py:129-137).  nterms sweeps of
 * the GEMM; 26 reach fp32 resolution.  Used for iteration 0, whose rho serves that one iteration only. */
int effq_prox_solve_shifted(const float* B0, const float* Ainv, const float* W0, const float* b0, const float* G,
                            const float* dual, int c2, int n, int has_bias, double rho, double eta,
                            double rho_inv, int nterms, float* wstar, float* bstar, void* ws, size_t ws_bytes,
                            void* stream);

/* ---- a4: ADMM elementwise steps (EfficientQConv.py:108-111,129-137,139-142) ----
 * v = wstar + dual                                  (input of the weight projection) */
int effq_admm_presum(const float* wstar, const float* dual, float* v, size_t n, void* stream);
/* G = f32(alpha)*b with b=f32(discretize(f64(v)/alpha,-1,1)); dual = (wstar - G + dual) / dual_div.
 * dual_div is 1, or 2 / (rho_max/rho) on the rho-schedule iterations (i % 50 == 0).  alpha from state_dev.
 * 2 <= levels <= 256, with or without Gq_out: the fp32 screen that finds the level of most values is exact up to there
 * (csrc/fp_level.h).  The same bound holds for every fixed point and statistics pass above that uses the screen:
 * effq_alpha_stats_f64, effq_alpha_fixed_point, effq_fixed_point_small, effq_fixed_point_coop(_rec) (their level
 * tallies are sized for it too), as it does for the bucket, bracket, trajectory and channel fixed points. */
int effq_admm_project_dual(const float* v, const float* wstar, const effq_fp_state* state_dev, int levels,
                           float* G, float* dual, float dual_div, int8_t* Gq_out, size_t n, void* stream);
/* Gq_out (optional): the int8 operand of the exact-integer convs below.  levels <= 128: the signed level numerator
 * j' = 2*level-(L-1) itself, so that G = alpha_w*j'/(L-1); 129 <= levels <= 256, where j' no longer fits: level-128,
 * i.e. j' = 2*(level-128) + (257-L); conv3d_calib_step_i8s takes that encoding at 256 levels only (+ 1). */
/* ---- the entry point north_star names ------------------------------------------------
 * One ADMM iteration's device work (EfficientQConv.py:118-122,161-165; PTQConv.py:154-167):
 * out = conv3d(xq, G, bias) in fp32 on the matrix cores (f32 MFMA, exact fp32 fma chains),
 * fused with sqerr_out[0] = sum (out-y)^2 and sqerr_out[1] = sum att*(out-y)^2 (fp64 scalars).
 * y_fp may be NULL (plain forward), out may be NULL (loss only), att may be NULL (sqerr[1]=sqerr[0]).
 * If act_alpha_dev != NULL the fp32 quant-dequant of PTQConv._quantize_act (levels act_levels,
 * range [0,1]) is applied to x while staging it (quantised forward, PTQConv.py:163-167).
 * ws: effq_conv_ws_bytes(geom) bytes, ZERO-FILLED once by the caller (it holds the ticket of the last-block
 * reduction, which every launch leaves at zero again; the same holds for the i8 conv workspaces below). */
size_t effq_conv_ws_bytes(const effq_geom* g);
int conv3d_quant_calib_step(const float* xq_ndhwc, const float* G, const float* bias, const float* y_fp,
                            const float* att, const effq_geom* g, const float* act_alpha_dev, int act_levels,
                            double* sqerr_out, float* out, void* ws, size_t ws_bytes, void* stream);
/* The launch conv3d_quant_calib_step makes for a geometry, answered on the host (no device, nothing launched).
 * loss_only != 0: a call with targets and no output, no mask and no fused quantiser, the only one the direct-gather
 * kernels take.  kind: 0 a tiled kernel (k_conv3d_k3 when fast, else k_conv3d), 1 k_conv3d_c4h<S>, 2 k_conv1_mfma,
 * 3 k_conv3d_c1h<SD, SH, SW>, 4 k_conv3d_c4.  kind 0: cslab channels per LDS slab, nslab slabs per tile, nt 32-channel
 * output blocks per wave, the grid, the 4 x 4 x 8-voxel output tiles and the dynamic LDS bytes.  kind != 0: fast, cslab,
 * nslab, nt and lds_bytes are 0, grid_y is 1 and ntiles counts what the kernel walks (4 x 4 x 8 tiles for 1 and 3, 32-voxel
 * wave tiles for 4, 16-voxel wave tiles for 2).  A geometry the planner refuses returns its error (effq_last_error). */
int effq_conv_plan_query(const effq_geom* g, int loss_only, int* kind, int* fast, int* cslab, int* nslab, int* nt,
                         int* grid_x, int* grid_y, int* ntiles, long long* lds_bytes);

/* ---- exact-integer ("int-simulated") form of the per-iteration loss evaluation -------------------
 * Same quantity as conv3d_quant_calib_step(xq, G, bias, y_fp, NULL, ...)'s sqerr_out[0], for quantised
 * activations and projected weights: x = alpha_a*k/(La-1) with level ids k (uint8, NDHWC) and
 * G = alpha_w*j'/(Lw-1) with Gq = j' (int8, reference weight layout).  The contraction runs on the i8
 * matrix cores with exact int32 accumulation; out = f32(alpha_a)*f32(alpha_w)/((La-1)(Lw-1)) * acc + bias.
 * Supported: 3x3x3, stride 1, C1 in {32,64,128,256,512}, C2 % 32 == 0, levels <= 128 (query effq_conv_i8_supported).
 * alpha_a: device float; alpha_w: w_state_dev->alpha.  sqerr_out[0] = sqerr_out[1] = sum (out-y)^2. */
int effq_conv_i8_supported(const effq_geom* g, int act_levels, int w_levels);
size_t effq_conv_i8_ws_bytes(const effq_geom* g);
int conv3d_calib_step_i8(const uint8_t* xidx_ndhwc, const int8_t* Gq, const float* bias, const float* y_fp,
                         const effq_geom* g, const float* act_alpha_dev, int act_levels,
                         const effq_fp_state* w_state_dev, int w_levels, double* sqerr_out, void* ws,
                         size_t ws_bytes, void* stream);
/* The quantised FORWARD of a calibrated layer on the same kernels (PTQConv.py:160-167 with quantised input and weights,
 * and the final loss of EfficientQConv.py:161-166 from the same pass): out (fp32, NDHWC) = the conv output, sqerr_out[0] =
 * sum (out - y)^2, sqerr_out[1] = sum att * (out - y)^2 (att: one weight per output voxel, [N][OD][OH][OW], or NULL: the
 * plain sum).  An exact integer contraction and ONE fp32 multiply-add per output instead of c1 k^3 fp32 products: what
 * the f32 conv of conv3d_quant_calib_step computes, without its rounding.  32 -> 32 and 64 -> 64 channels on volumes the
 * kernels' tiles divide (effq_conv_i8_out_supported); ws as for conv3d_calib_step_i8. */
int effq_conv_i8_out_supported(const effq_geom* g, int act_levels, int w_levels);
int conv3d_quant_forward_i8(const uint8_t* xidx_ndhwc, const int8_t* Gq, const float* bias, const float* y_fp,
                            const float* att, const effq_geom* g, const float* act_alpha_dev, int act_levels,
                            const effq_fp_state* w_state_dev, int w_levels, double* sqerr_out, float* out, void* ws,
                            size_t ws_bytes, void* stream);
/* The launch conv3d_calib_step_i8 (want_out == 0) or conv3d_quant_forward_i8 (want_out != 0) makes for a geometry, answered
 * on the host.  kernel: 1 k_conv3d_i8l2e, 2 k_conv3d_i8l2, 3 k_conv3d_i8<2>, 4 k_conv3d_i8w, 5 k_conv3d_i8g<4>,
 * 6 k_conv3d_i8g<8>, 7 k_conv3d_i8g2<16>; ntiles: output tiles of 8 x 4 x 8 (C1 = 32), 2 x 4 x 8 (C1 = 512) or 4 x 4 x 8
 * voxels.  An output no kernel can store is an error. */
int effq_conv_i8_plan_query(const effq_geom* g, int want_out, int* kernel, int* grid_x, int* grid_y, int* ntiles);

/* The same exact-integer loss for the layers the tiled kernels above do not take: few taps*channels
 * (KD*KH*KW*C1 <= 256 with C1 == 4 or C1 % 16 == 0: the first conv, the 1x1x1 convs, the classifier), any
 * stride/padding, up to 256 activation levels, and up to 128 or exactly 256 weight levels (q_first/q_last = 256 in the
 * reference's recipes).  Gq holds the int8 operands effq_admm_project_dual emits (2*level-(Lw-1), or level-128 at Lw = 256).
 * prepare != 0 (first call of a layer) also rebuilds the per-voxel level sums the Lw > 128 form needs; they
 * live in ws between calls.  ws: effq_conv_i8s_ws_bytes(geom, act_levels, w_levels). */
int effq_conv_i8s_supported(const effq_geom* g, int act_levels, int w_levels);
size_t effq_conv_i8s_ws_bytes(const effq_geom* g, int act_levels, int w_levels);
int conv3d_calib_step_i8s(const uint8_t* xidx_ndhwc, const int8_t* Gq, const float* bias, const float* y_fp,
                          const effq_geom* g, const float* act_alpha_dev, int act_levels,
                          const effq_fp_state* w_state_dev, int w_levels, int prepare, double* sqerr_out,
                          void* ws, size_t ws_bytes, void* stream);
/* The launch conv3d_calib_step_i8s makes, answered on the host: nj K steps of 32 x ct column tiles of 32 channels, the taps
 * and K = taps * C1, the activation offset aoff (128 above 128 levels) and the weight multiplier wmul (2 at 256 levels),
 * and the grid.  An unsupported geometry or level pair is an error. */
int effq_conv_i8s_plan_query(const effq_geom* g, int act_levels, int w_levels, int* nj, int* ct, int* taps, int* k,
                             int* aoff, int* wmul, int* grid);

/* ---- f3: tune_activation_range (ptqer.py:238-272) - Adam on every alpha_act, end-to-end MSE, STE through discretize ----
 * Backward of q = discretize(x / alpha, L, 0, 1) * alpha (PTQConv.py:114-116; round with identity gradient,
 * layer_helper.py:13-22; clamp with torch's inclusive mask) given gq = dLoss/dq:
 *   gx_out = gq * mask (may be NULL),  *galpha_out (device double) = sum gq * (r - mask * x / alpha).
 * ws: the reduction workspace (effq_reduce_ws_bytes()).  The input gradient of the conv itself is the conv entry point
 * applied to the output gradient with flipped, transposed weights (stride 1). */
int effq_act_quant_backward(const float* x, const float* alpha_dev, int levels, const float* gq, float* gx_out,
                            double* galpha_out, size_t n, void* ws, void* stream);
/* torch.optim.Adam step (no weight decay, no amsgrad) on n parameters; t = step number starting at 1.  The hyper-parameters
 * are doubles: 1 - beta, the bias corrections 1 - beta^t and lr / (1 - beta1^t) are formed in double, as torch forms them
 * from Python floats, and rounded to fp32 once.  n = 0 is a no-op. */
int effq_adam_step(float* p, const float* g, float* m, float* v, double lr, double b1, double b2, double eps,
                   int t, size_t n, void* stream);

/* ---- the whole ADMM loop of a layer in ONE call (EfficientQConv.py:99-144) -----------------------------------
 * Enqueues `iters` iterations of { prox solve, weight-scale fixed point, projection + dual update } on stream_main,
 * the loss of each iterate (conv + squared error against y_fp, the reference's per-iteration F.conv3d + F.mse_loss)
 * on stream_loss one iteration behind, and the inverses of A(rho) for the later rho values on stream_side.  stream_loss
 * / stream_side may be NULL (that work then runs on stream_main).  No host synchronisation; on return stream_main is
 * ordered after everything the call enqueued on the other two.
 * Results are kept PER ITERATION (slot i of each ring is written once and never reused, so the three streams need no
 * back-pressure): G_ring [iters][nw] projected weights, Gq_ring [iters][nw] their int8 operands (required for
 * loss_kind 1/2, else may be NULL), b_ring [iters][c2] (NULL without bias), state_ring [iters] scale states
 * (state_ring[iters-1].alpha is the reference's final alpha_w, quirk Q6), hist [iters][2] = {sum (out-y)^2, same}.
 * The best iterate is chosen afterwards by effq_admm_select_best(); a data-parallel caller all-reduces hist first
 * (ONE collective per layer for the 200 per-iteration losses).
 * rho schedule: after iteration i with i % rho_period == 0, rho doubles while 2*rho <= rho_max (else rho = rho_max)
 * and dual is divided by the same factor (EfficientQConv.py:129-137).  One inverse per distinct rho that serves more
 * than one iteration: ainv_pool holds n_ainv >= effq_admm_num_inverses(...) matrices of n*effq_ainv_ld(n) floats.
 * loss_kind: 0 = conv3d_quant_calib_step on xq (fp32), 1 = conv3d_calib_step_i8, 2 = conv3d_calib_step_i8s (both on
 * xidx, act_alpha_dev, act_levels), 4 = effq_gram_loss (no pass over the voxels; loss_Au / loss_Bu / loss_syy below).  Workspaces as the respective entry points document them (conv_ws zero-filled
 * once; red_ws = the reduction workspace; fp_ws = effq_fp_bucket_ws_bytes(nw), may be NULL -> cooperative fixed point;
 * inv_ws / inv_ws_side = effq_spd_inverse_ws_bytes(n) each, the second only with stream_side).
 * *err_flag (device int32, zeroed by the caller) is set when a weight fixed point hits its cap (layer_helper.py:62-64). */
typedef struct effq_admm_run_args {
  const float* A0; const float* B0; const float* W0; const float* b0;
  int32_t c2, n, has_bias, w_levels;
  int32_t iters, rho_period;
  double rho, rho_max, eta, tol;
  effq_geom geom;
  int32_t loss_kind, act_levels;
  const float* xq; const uint8_t* xidx; const float* y_fp; const float* act_alpha_dev;
  float* dual; float* wstar; float* v;
  float* G_ring; int8_t* Gq_ring; float* b_ring; effq_fp_state* state_ring; double* hist;
  int32_t* err_flag;
  float* ainv_pool; int32_t n_ainv;
  void* prox_ws; size_t prox_ws_bytes;
  void* red_ws;
  void* fp_ws; size_t fp_ws_bytes;
  /* effq_fixed_point_traj for the weight projection (where effq_admm_uses_traj(weights, w_levels) says so): fp_pred =
   * effq_fp_traj_pred_bytes() of device memory (the run zero-fills it), fp_traj_ws = effq_fp_traj_ws_bytes(weights),
   * zero-filled once.  NULL: the older fixed points only. */
  void* fp_pred; void* fp_traj_ws; size_t fp_traj_ws_bytes;
  void* inv_ws; size_t inv_ws_bytes;
  void* inv_ws_side; size_t inv_ws_side_bytes;
  void* conv_ws; size_t conv_ws_bytes;
  void* stream_main; void* stream_loss; void* stream_side;
  /* optional second side stream with its own inverse workspace: the later inverses alternate between the two side
   * streams (their serial pivot phases overlap); NULL: one side stream */
  void* stream_side2; void* inv_ws_side2; size_t inv_ws_side2_bytes;
  /* loss_kind 4: the loss of an iterate from the layer's unweighted Gram system (effq_gram_loss): Au [n][n], Bu [c2][n]
   * (effq_gram_accum_i8_unw), syy = one device double, sum y^2 over this rank's voxels; conv_ws = effq_gram_loss_ws_bytes(n)
   * zero-filled once.  NULL for the other kinds. */
  const double* loss_Au; const double* loss_Bu; const double* loss_syy;
  /* loss_kind 5: the same from effq_gram_loss_i8, in the groups the loss stream picks the iterates up in: loss_Au / Bu / syy
   * as above, loss_planes / loss_nplanes from effq_gram_loss_i8_prepare, Gq_ring and act_alpha_dev as for loss_kind 1;
   * conv_ws = effq_gram_loss_i8_ws_bytes() zero-filled once. */
  const int8_t* loss_planes; int32_t loss_nplanes;
  /* lwq_verbose (EfficientQConv.py:114-127): iters x 2 device doubles, sum (w* - G)^2 and sum (G - G_prev)^2 of every
   * iteration (the primal residual is the root of the first, the dual residual rho times the root of the second); NULL: not
   * computed (one small launch per iteration) */
  double* res_ring;
  /* channel mode (lwq_channel_wise: one weight scale per output channel): channel_wise != 0 runs the weight projection
   * through effq_fixed_point_channels_proj instead of the per-tensor fixed points; alpha_ring [iters][c2] device doubles
   * receive every iteration's scales, w_iters_ring [iters][c2] int32 the per-row fixed-point iteration counts.
   * state_ring is then not written.  Only loss_kind 0 and 4 (they take G as fp32 values); 1, 2, 5 -> EFFQ_ERR_ARG. */
  int32_t channel_wise;
  double* alpha_ring; int32_t* w_iters_ring;
} effq_admm_run_args;
/* 1 if effq_admm_run takes the trajectory weight projection (effq_fixed_point_traj) for a layer of nw weights at
 * w_levels levels - the caller then passes fp_pred (effq_fp_traj_pred_bytes(), zero-filled) and fp_traj_ws
 * (effq_fp_traj_ws_bytes(nw)); otherwise both may be NULL and nothing needs to be allocated. */
int effq_admm_uses_traj(size_t nw, int w_levels);
int effq_admm_num_inverses(double rho, double rho_max, int iters, int rho_period);
int effq_admm_run(const effq_admm_run_args* a);
/* best = the EARLIEST iterate with the smallest hist[i][0] ("if i == 0 or lossf < best", EfficientQConv.py:139-142):
 * copies its G / b* out of the rings; best_out[0] = its loss sum, best_out[1] = its index (as a double). */
int effq_admm_select_best(const double* hist, int iters, const float* G_ring, const float* b_ring, size_t nw, size_t nb,
                          float* best_G, float* best_b, double* best_out, void* stream);

/* ---- the Gram system as ONE data-parallel message ------------------------------------------------------------------
 * A0 is symmetric: a rank's partial sums travel as [upper triangle of A0, row-major: n(n+1)/2 floats | B0: c2*n floats]
 * (effq_gram_packed_elems), one all-reduce per layer instead of two and half the bytes of the full matrix
 * (solver.py:302-312 sums the per-sample contributions the same way).  unpack mirrors the triangle back. */
size_t effq_gram_packed_elems(int n, int c2);
int effq_gram_pack(const float* A0, const float* B0, int n, int c2, float* buf, void* stream);
int effq_gram_unpack(const float* buf, int n, int c2, float* A0, float* B0, void* stream);

/* ---- measurement aid: sampling profiler of effq_admm_run (off by default, per host thread) ---------------------
 * effq_prof_enable(every > 0): from now on every `every`-th iteration of effq_admm_run brackets its ops with HIP-event
 * pairs recorded on the stream the op is launched on; effq_prof_enable(0) stops and drops the records.  After the
 * caller has synchronised the device, effq_prof_read(i) returns record i: kind 1 prox solve, 2 weight-scale fixed point,
 * 3 projection + dual update, 4 loss evaluation (conv + squared error, with its weight pack), 5 inverse of A(rho)
 * (iter < 0); ms = elapsed time between the two events. */
typedef struct effq_prof_record {
  int32_t kind, iter, loss_kind, c2, n;
  effq_geom geom;
  float ms;
} effq_prof_record;
int effq_prof_enable(int every);
int effq_prof_count(void);
int effq_prof_read(int i, effq_prof_record* out);

/* ---- glue between the quantised convs (row a11): x2 trilinear up-sampling of the decoder (factory_blk.py:70-93,
 * nn.Upsample(scale_factor, mode='trilinear'), align_corners = False) on NDHWC tensors; per-axis scale 1 or 2. */
int effq_upsample_trilinear(const float* x_ndhwc, int N, int D, int H, int W, int C, int sd, int sh, int sw,
                            float* y_ndhwc, void* stream);

/* ---- f2: bit-packed storage of level ids ---------------------------------------------------
 * The reference stores one uint8 per weight (store_int_weight, PTQConv.py:125-152); these pack the level ids
 * at 1/2/4/8 bits each (little-endian bit stream: element i in bits [i*bits, (i+1)*bits)) and back. */
size_t effq_packed_bytes(size_t n, int bits);
int effq_pack_levels(const uint8_t* idx, size_t n, int bits, uint8_t* packed, void* stream);
int effq_unpack_levels(const uint8_t* packed, size_t n, int bits, uint8_t* idx, void* stream);

/* ---- validation on whole volumes (evaluate.validate_seg; utils/validate.py:212-264, utils/transforms.py:784-852,
 * utils/metrics.py) -------------------------------------------------------------------------------------------------
 * Windows of extent (pd, ph, pw) and overlap (od, oh, ow) < extent: along each axis the starts step by extent - overlap
 * while a whole window still ends strictly before the border, then one window lies flush with it; windows are numbered
 * in (d, h, w) raster order (evaluate.window_starts / image_to_patch3d).
 *
 * A flip mask is 0..7: bit 0 mirrors d, bit 1 mirrors h, bit 2 mirrors w; a mirrored axis maps window-local index z to
 * p - 1 - z.  The three window entry points (window.hip) have one owner thread per destination element and no atomics:
 * equal inputs give equal bits.
 *
 * Gather: vol (N, C, D, H, W) -> out (count, N, pd, ph, pw, C), windows first .. first + count - 1, channels-last, the
 *   content of every window mirrored along the axes of `flip`.  flip outside 0..7: EFFQ_ERR_ARG.
 * Put: src (count, C, pd, ph, pw), a network's last head with count = windows * N, un-mirrored into dst (count, pd, ph,
 *   pw, C), a slice of the stitch's window buffer:  dst[m, z, y, x, c] = (accumulate ? dst[m, z, y, x, c] : 0) +
 *   src[m, c, flip(z), flip(y), flip(x)], one fp32 add; accumulate = 0 copies the bits.  C <= 8, count C pd ph pw < 2^31.
 * Stitch: win (nwin, N, pd, ph, pw, C) holding the sum of nflip >= 1 passes over every window -> out (N, C, D, H, W),
 *   C <= 8.  wd, wh, ww all NULL: each voxel is the sum of its covering windows in raster order over ((float)nflip times
 *   their count); with nflip = 1 bit for bit evaluate.patch_to_image3d.  All three given, pd, ph, pw fp32 per-axis
 *   weights on the device: over the covering windows in raster order  wgt = (wd[z] wh[y]) ww[x], acc[c] += wgt win[..],
 *   wsum += wgt  in fp32, then out = acc[c] / ((float)nflip wsum).  With all weights 1.0f and any nflip that is the bits
 *   of the unweighted stitch (every product is its addend, the weight sum is the exact count).  Some but not all of
 *   wd, wh, ww NULL, nflip < 1 or C > 8: EFFQ_ERR_ARG.
 * Tallies: logits (C, S) of one case and its label -> counts (C, 4) int64 = TP, FP, FN, TN per class.
 *   EFFQ_SEG_ARGMAX: label (S) class ids; prediction = the first largest channel (torch.max).
 *   EFFQ_SEG_SIGMOID: label (C, S) 0/1; channel c predicted when logit >= thresh, where thresh is the least float at
 *   which the framework's fp32 sigmoid reaches 0.5; then merged across channels by `fuse` (misc.merge_label_basic:
 *   AGG p[i] = any(p[i:]), CON p[i] = all(p[:i+1])).  ws: EFFQ_SEG_TALLIES_WS_BYTES of scratch. */
#define EFFQ_SEG_TALLIES_MAX_CLASSES 8
#define EFFQ_SEG_TALLIES_WS_BYTES (1024 * 3 * EFFQ_SEG_TALLIES_MAX_CLASSES * 4)
enum { EFFQ_SEG_ARGMAX = 0, EFFQ_SEG_SIGMOID = 1 };
enum { EFFQ_SEG_FUSE_NONE = 0, EFFQ_SEG_FUSE_AGG = 1, EFFQ_SEG_FUSE_CON = 2 };
int effq_window_gather(const float* vol, int N, int C, int D, int H, int W, int pd, int ph, int pw, int od, int oh,
                       int ow, int first, int count, int flip, float* out, void* stream);
int effq_window_put(const float* src, int count, int C, int pd, int ph, int pw, int flip, int accumulate, float* dst,
                    void* stream);
int effq_window_stitch(const float* win, int N, int C, int D, int H, int W, int pd, int ph, int pw, int od, int oh,
                       int ow, const float* wd, const float* wh, const float* ww, int nflip, float* out, void* stream);
int effq_seg_tallies(const float* logits, const uint8_t* label, int C, long long S, int mode, int fuse, float thresh,
                     long long* counts, void* ws, size_t ws_bytes, void* stream);

/* Threshold sweep of one case (validate_seg(..., sweep=True), --thr_sweep): logits (C, S), label, mode and fuse as
 * effq_seg_tallies -> hist (C, 2, EFFQ_SEG_SWEEP_BINS) int64 on the device, overwritten: hist[c][g][b] = the voxels with
 * truth g for class c (the gt bit of the tallies' decision) whose score for class c falls in bin b.
 *   Scores, fp32, nothing fused.  EFFQ_SEG_SIGMOID: NONE s_c = x_c; AGG s_c = the largest non-NaN of x_c .. x_{C-1} (NaN
 *   when all are NaN); CON s_c = the least of x_0 .. x_c (NaN when any is NaN).  EFFQ_SEG_ARGMAX: s_c = x_c - max_{j != c}
 *   x_j, one subtraction, the max with NaN as the largest value (torch.max), so a NaN in another channel makes s_c NaN;
 *   C = 1: s_0 = x_0.
 *   Edges: e_0 = -inf, e_k = (k - 2048) / 128 for k = 1 .. 4095, except e_2048 = thresh in sigmoid mode (it must lie
 *   strictly between e_2047 and e_2049) and 0 in argmax mode, where thresh is not read.  bin(s) = the number of k >= 1
 *   with e_k <= s; NaN -> 0.  In sigmoid mode bin >= 2048 is the tallies' decision at `thresh`.  In argmax mode the bin is
 *   then pinned to the tallies' decision: max(bin, 2048) for the predicted class, min(bin, 2047) for every other.
 *   The counts TP, FP, FN, TN of "score >= e_k" are the sums of hist[c][1][k:], hist[c][0][k:], hist[c][1][:k],
 *   hist[c][0][:k]; row 2048 is what effq_seg_tallies returns.
 * 1 <= C <= EFFQ_SEG_TALLIES_MAX_CLASSES, 0 < S < 2^31, fuse NONE in argmax mode, logits 4-B and hist 8-B aligned;
 * anything else returns EFFQ_ERR_ARG before a launch and leaves hist untouched.  Workgroup-private 32-bit counters in
 * LDS, flushed with 64-bit integer atomics into hist, which a first launch zeroes: integer adds only, so equal inputs
 * give equal bits.  Two launches on `stream`, no read by the host, no workgroup that waits for another.
 * effq_seg_sweep_edges: the EFFQ_SEG_SWEEP_BINS edges of a mode and thresh into host memory, index 0 = -inf.
 * effq_seg_sweep_plan: the launch effq_seg_sweep makes; launches nothing.  *grid workgroups (voxel ranges x
 * ceil(C / 2) class pairs), each of which makes *trips trips over its groups of four voxels (0 when S < 4). */
#define EFFQ_SEG_SWEEP_BINS 4096
int effq_seg_sweep(const float* logits, const uint8_t* label, int C, long long S, int mode, int fuse, float thresh,
                   long long* hist, void* stream);
int effq_seg_sweep_edges(int mode, float thresh, float* edges_host);
int effq_seg_sweep_plan(int C, long long S, int mode, int* grid, int* trips);

/* Agreement of two networks on one case (validate_seg(..., fp_model=...), --vs_fp): logits_q and logits_fp, the stitched
 * last-head logits (C, S) fp32 of the calibrated and of the full-precision network; mode, fuse and thresh as
 * effq_seg_tallies, and both networks' voxels are decided by the tallies' own rule.  One pass over the 2 C S floats:
 *   counts (C, 4) int64 = both, Q only, FP only, neither: TP, FP, FN, TN with the FP network's decision as the truth.
 *   flips  (1)    int64 = the voxels where the decision of at least one class differs.
 *   stats  (C, 4) fp64  = sum (q - f)^2, sum f^2, max |q - f|, sum |p_q - p_f| per class, differences and squares formed
 *          in fp64 from the fp32 logits; p is in fp64 the sigmoid of the channel (before `fuse`) for EFFQ_SEG_SIGMOID and
 *          the softmax over the C channels for EFFQ_SEG_ARGMAX.
 *   map    (S) uint8, or NULL: bit c set where the decision of class c differs.
 * Per-workgroup partials, then one workgroup adds them in block order; no floating-point atomics, so equal inputs give
 * equal bits.  16-B loads for the first 4 (S / 4) voxels of every channel whatever S is, the last S % 4 voxels one by one.
 * Two launches on `stream`, no read by the host, no workgroup that waits for another.  ws: EFFQ_SEG_AGREEMENT_WS_BYTES of
 * scratch, 8-B aligned. */
#define EFFQ_SEG_AGREEMENT_WS_BYTES (768 * (4 * EFFQ_SEG_TALLIES_MAX_CLASSES * 8 + (3 * EFFQ_SEG_TALLIES_MAX_CLASSES + 1) * 4))
int effq_seg_agreement(const float* logits_q, const float* logits_fp, int C, long long S, int mode, int fuse,
                       float thresh, long long* counts, long long* flips, double* stats, uint8_t* map, void* ws,
                       size_t ws_bytes, void* stream);

/* Labels: logits (N, C, S) of N cases -> one label map (N, S) of out_bytes = 1 (uint8) or 2 (uint16) per voxel, or
 * for EFFQ_SEG_LABEL_PLANES the C merged 0/1 planes (N, C, S) uint8.  The per-voxel decisions are the tallies': the
 * ARGMAX rule uses EFFQ_SEG_ARGMAX (fuse must be NONE), every other rule EFFQ_SEG_SIGMOID with `thresh` and `fuse`.
 *   ARGMAX: the class id (metrics.get_pred_lits).
 *   BRATS:  misc.merge_label_brats of the merged channels: 0; 1 where ch0; 2 where ch0 and not ch1; 4 where ch2
 *           (later assignments win).  C >= 3.
 *   RANK:   i + 1 of the highest set channel, 0 when none (fuse CON: metrics.get_pred_brats_con_merge).
 *   PLANES: the merged channels themselves (misc.merge_label_basic).  out_bytes = 1. */
#define EFFQ_SEG_LABEL_ARGMAX 0
#define EFFQ_SEG_LABEL_BRATS 1
#define EFFQ_SEG_LABEL_RANK 2
#define EFFQ_SEG_LABEL_PLANES 3
int effq_seg_labels(const float* logits, int N, int C, long long S, int rule, int fuse, float thresh, int out_bytes,
                    void* out, void* stream);

/* Labels on the source grid (the `predict` mission, predict.py): the stitched logits (C, box) of one subject live on
 * the box pmin <= (d, h, w) < pmin + box of the working grid `grid`, which effq_prep_resample made from the source grid
 * `source` with `factors` = target spacing / source spacing per axis (1 without resampling).  out (source) uint8 gets
 * one label per source voxel.  Per axis, source index s, in fp64: t = (s + 0.5) / factor (a division); the voxel is
 * inside iff pmin <= min(floor(t), grid - 1) < pmin + box on all three axes, and is 0 otherwise; inside, q = clamp(t -
 * 0.5 - pmin, 0, box - 1), i0 = floor(q), i1 = min(i0 + 1, box - 1), l1 = float(q - i0), l0 = 1.0f - l1, and each
 * logit is combined in fp32 in the order of EFFQ_PREP_LINEAR, nothing fused.  The C values are decided and mapped to a
 * label as effq_seg_labels does for `rule` (ARGMAX, BRATS or RANK; PLANES is an argument error: C planes have no place
 * on a source grid), `fuse` and `thresh`.  box, pmin, grid, source (three ints each) and factors (three doubles) are
 * host memory, read before the call returns.  1 <= C <= EFFQ_SEG_TALLIES_MAX_CLASSES; every extent <= 32767, the
 * voxels of source, of grid and of the C box planes together < 2^31 each; 0 <= pmin, pmin + box <= grid; factors in
 * (0, 1e6].  One launch, no atomics, no reductions: equal inputs give equal bits. */
int effq_seg_labels_source(const float* logits, int C, const int* box, const int* pmin, const int* grid,
                           const double* factors, const int* source, int rule, int fuse, float thresh, uint8_t* out,
                           void* stream);

/* Probabilities and an uncertainty on the source grid (`predict --save_prob / --save_unc`): logits, C, box, pmin, grid,
 * factors and source as effq_seg_labels_source, with its argument checks; v_c, the logit of channel c at a source
 * voxel, is interpolated exactly as there (the same fp64 axis arithmetic, inside rule and fp32 corner order).  probs
 * (C, source) uint8 and unc (source) uint8 hold rintf(255 x), half to even, a NaN x as 0; either may be null, not both.
 *   EFFQ_SEG_ARGMAX:  p_c = exp(v_c - m) / S with m = max v and S = sum_c exp(v_c - m); u = (ln S - sum_c p_c (v_c - m))
 *                     / ln C, the entropy over the C classes as a share of its maximum; C = 1: p = 1, u = 0.  Channels
 *                     equal to an infinite m count as v_c - m = 0 (k channels at +inf: 1 / k each).
 *   EFFQ_SEG_SIGMOID: p_c = 1 / (1 + exp(-v_c)) per raw channel (no merge, no threshold); u = max_c h(v_c), the binary
 *                     entropy of p_c in bits, computed from |v_c|.
 * Outside the box: SIGMOID every channel 0, ARGMAX channel 0 = 255 and the others 0; u = 0.  fp32 with expf, logf and
 * true divisions: 255 p within 5e-4 and 255 u within 1e-3 of the exact value of the fp32 v_c, before the rounding to a
 * level.  With probs, C times the voxels of source < 2^31.  One launch, no atomics, no reductions: equal inputs give
 * equal bits. */
int effq_seg_probs_source(const float* logits, int C, const int* box, const int* pmin, const int* grid,
                          const double* factors, const int* source, int mode, uint8_t* probs, uint8_t* unc, void* stream);

/* ---- connected components of 0/1 volumes and the lesion-level columns of the validation (validate_seg(..., is_cc=True):
 * utils/validate.py:28-36, utils/metrics.py:69-94: num_component, num_false_positive, num_positive, num_false_negative,
 * there with scipy.ndimage.label on the host).  Block-based union-find: tiles of 8 x 8 x 32 voxels are labelled in LDS,
 * the tiles are joined across their faces, edges and corners by a lock-free atomicMin union on the label array, every
 * voxel is pointed at its root and the roots are counted.  Five launches (with the masks and the zeroing of the flags
 * of effq_seg_lesions: seven), all on `stream`, no read by the host and no workgroup that waits for another.
 *
 * effq_cc_label: masks (P, D, H, W) uint8, non-zero = foreground -> labels (P, D, H, W) int32: 0 for background, for a
 *   foreground voxel 1 + the least linear index (d*H*W + h*W + w) of any voxel of its component; ncomp (P) = the number
 *   of components of each mask.  The label does not depend on the order of the unions: equal inputs give equal bits, and
 *   numbering the distinct labels in raster order gives scipy.ndimage.label's.  connectivity 26 (the full 3 x 3 x 3
 *   neighbourhood, the 3-D counterpart of the np.ones((3, 3)) of metrics.py) or 6 (faces only, scipy's default).
 *   P * D*H*W < 2^31, P <= 65535.
 * effq_seg_lesions: stitched logits (C, D, H, W) of one case and its label, arguments as effq_seg_tallies -> counts
 *   (C, 4) int64 per class: totall = components of the label mask (num_positive), predl = components of the predicted
 *   mask, fnl = label components without a predicted voxel (num_false_negative), fpl = predicted components without a
 *   labelled voxel (num_false_positive).  The masks are the tallies' own decisions (in argmax mode class 0, the
 *   background, is a class like any other); the 2 C masks are labelled by the same launches.
 * ws: effq_cc_ws_bytes(P, D, H, W) bytes for either call, P = 2 C for effq_seg_lesions: 4 B of label, 1 B of overlap flag
 *   per plane and voxel, 2 B of decision bits per voxel and the partial counts (effq_cc_label keeps its labels in
 *   `labels` and uses the partial counts only).  A BraTS case (3 classes, 155 x 240 x 240): 6 planes x 8.9 M x 4 B =
 *   214 MB of labels, 286 MB in all. */
size_t effq_cc_ws_bytes(int P, int D, int H, int W);
int effq_cc_label(const uint8_t* masks, int P, int D, int H, int W, int connectivity, int32_t* labels,
                  long long* ncomp, void* ws, size_t ws_bytes, void* stream);
int effq_seg_lesions(const float* logits, const uint8_t* label, int C, int D, int H, int W, int mode, int fuse,
                     float thresh, int connectivity, long long* counts, void* ws, size_t ws_bytes, void* stream);

/* ---- one record per connected component (validate_seg(..., lesion_table=True): which lesions were missed or invented,
 * and how big; the reference carries sizeL / sizeP, utils/metrics.py:48-52, but only ever sums them over a mask).  After
 * the five launches of effq_cc_label (seven of effq_seg_lesions) four more, on the same labels: the roots of every chunk
 * of EFFQ_CC_TABLE_CHUNK consecutive voxels are counted, the chunk counts of each plane are scanned, every chunk is
 * walked again to give its roots their rows, and every foreground voxel adds itself to its component's row (equal rows
 * of a wave combined, the sums of a workgroup kept in LDS).  All on `stream`, no read by the host and no workgroup that
 * waits for another; integer adds only, so equal inputs give equal bits.
 *
 * Order: row k of a plane is the component whose first voxel (least linear index d*H*W + h*W + w) is the k-th smallest -
 *   component k + 1 of scipy.ndimage.label.
 * effq_cc_table: masks as effq_cc_label -> rows (P, max_rows, 2) int32 = first voxel, size (voxels); nrows (P) = the
 *   number of components of each mask.
 * effq_seg_lesion_table: arguments as effq_seg_lesions -> counts (C, 4), bit for bit effq_seg_lesions'; nrows (2 C) and
 *   rows (2 C, max_rows, 3) int32 = first voxel, size, overlap.  Plane q < C is the predicted mask of class q, plane
 *   C + q its label mask; overlap = the voxels of the component that the other mask of its class holds too (0: a false
 *   positive lesion in a predicted plane, a missed lesion in a label plane).
 * Truncation: nrows is always the true count.  Of a plane with nrows > max_rows the first max_rows rows are written,
 *   complete; of a plane with fewer, rows nrows .. max_rows - 1 are left as they were.  Nothing is written past the table.
 * ws: effq_cc_table_ws_bytes(P, D, H, W, max_rows) bytes, P = 2 C for effq_seg_lesion_table: effq_cc_ws_bytes(P, D, H, W)
 *   (effq_cc_table keeps its labels there) and one counter per plane and chunk - 105 KB more for a BraTS case; nothing
 *   grows with max_rows today.  0 for dimensions out of range or max_rows <= 0.  Bad arguments (a null pointer,
 *   max_rows <= 0, a connectivity other than 6 or 26, dimensions out of range) return EFFQ_ERR_ARG, a short workspace
 *   EFFQ_ERR_WORKSPACE; both launch nothing. */
#define EFFQ_CC_TABLE_CHUNK 2048
size_t effq_cc_table_ws_bytes(int P, int D, int H, int W, int max_rows);
int effq_cc_table(const uint8_t* masks, int P, int D, int H, int W, int connectivity, int max_rows, int32_t* rows,
                  long long* nrows, void* ws, size_t ws_bytes, void* stream);
int effq_seg_lesion_table(const float* logits, const uint8_t* label, int C, int D, int H, int W, int mode, int fuse,
                          float thresh, int connectivity, int max_rows, long long* counts, long long* nrows,
                          int32_t* rows, void* ws, size_t ws_bytes, void* stream);

/* ---- the overlap of every (label lesion, predicted lesion) pair (validate_seg(..., lesion_match=True): one-to-one
 * matching, lesion F1, panoptic quality and lesion-wise Dice need it; the overlap column of the lesion table says how
 * many voxels of a lesion the other mask holds, not which lesion of it).  The launches of effq_seg_lesion_table and
 * four more: the hash tables are emptied, one streaming pass per class counts the voxels of every pair (equal pairs of a
 * wave combined, the sums of a workgroup kept in LDS, the rest into an open-addressing table of the class by a 64-bit
 * compare-and-swap and an add), the occupied slots are gathered and then put in order by their rank.  All on `stream`,
 * no read by the host, no workgroup that waits for another; integer adds only and an order that is the keys' own, so
 * equal inputs give equal bits.
 *
 * effq_seg_lesion_match: arguments as effq_seg_lesion_table, and max_pairs -> counts, nrows, rows: bit for bit
 *   effq_seg_lesion_table's (the same launches, the same truncation); npairs (C) int64 and pairs (C, max_pairs, 3)
 *   int32 = label row, predicted row, the voxels both components hold: one record per pair of a component of the label
 *   mask and a component of the predicted mask of class c that share a voxel.  A row is the 0-based row of the component
 *   in its plane of effq_seg_lesion_table (scipy.ndimage.label's number - 1), valid whether or not it fits max_rows:
 *   the pairs do not depend on max_rows.  Order: ascending in (label row, predicted row).
 * A class with more than max_pairs pairs: npairs[c] = -1 and its records are unspecified; nothing is written past the
 *   table and the other classes are what they would be.  Ask again with a larger max_pairs.
 * ws: effq_seg_lesion_match_ws_bytes(C, D, H, W, max_rows, max_pairs) bytes: effq_cc_table_ws_bytes(2 C, ...) and per
 *   class 16 B of words, 12 B for each of the T slots of the table (T = the least power of two >= 2 max_pairs, 256 or
 *   more) and 12 B for each of the max_pairs gathered records: 3 x (16 + 12 x 8192 + 12 x 4096) B = 442 KB more for a
 *   BraTS case at max_pairs 4096.  It may hold anything on entry.  0 for what the call refuses.
 * Bad arguments (those of effq_seg_lesion_table, max_pairs <= 0, C * max_pairs * 3 >= 2^31) return EFFQ_ERR_ARG, a
 *   short workspace EFFQ_ERR_WORKSPACE; both launch nothing and leave the outputs as they were. */
size_t effq_seg_lesion_match_ws_bytes(int C, int D, int H, int W, int max_rows, int max_pairs);
int effq_seg_lesion_match(const float* logits, const uint8_t* label, int C, int D, int H, int W, int mode, int fuse,
                          float thresh, int connectivity, int max_rows, int max_pairs, long long* counts,
                          long long* nrows, int32_t* rows, long long* npairs, int32_t* pairs, void* ws, size_t ws_bytes,
                          void* stream);

/* ---- cleaning a predicted label map by connected components (--post: keep the largest liver, relabel small specks; the
 * reference's merge_label_brats_inference, utils/misc.py, is the need, not the specification).  in (D, H, W) uint8 label
 * values -> out (D, H, W), which may be `in` itself.  R rules, 1 <= R <= EFFQ_LABEL_CLEAN_MAX_RULES, apply in order, each
 * to the map the previous one left.  Rule r: sets (R, 256) uint8 on the host, non-zero = the value is in the rule's mask
 * (sets[r][0] must be 0); rules (R, 3) long long on the host = op, N, TO.  Both host arrays are read before the call
 * returns.
 *   EFFQ_LABEL_CLEAN_LARGEST: the largest component of the mask stays, the voxels of every other become TO (N ignored).
 *     Of several largest components of equal size the one whose first voxel (least linear index d*H*W + h*W + w) is
 *     least stays.
 *   EFFQ_LABEL_CLEAN_MIN: the voxels of every component with fewer than N voxels become TO (N >= 1; size == N stays).
 *   TO is 0..255 and not in the rule's own set.  A rule whose mask is empty changes nothing.
 * stats (R, 2) int64 on the device: the components the rule's mask had, the voxels the rule relabelled.
 * Per rule: the membership plane (one launch), the five labelling launches of effq_cc_label on it, the component sizes
 *   added at the roots (equal roots of a wave combined before the atomic; int32, a plane holds < 2^31 voxels), for
 *   LARGEST one 64-bit atomicMax over the roots of size << 32 | (0xFFFFFFFF - root), and one pass that rewrites and
 *   counts: 8 launches for MIN, 9 for LARGEST, after one launch that zeroes the counters (and a device copy when out is
 *   not in).  All on `stream`, no read by the host and no workgroup that waits for another.  Integer adds and a max only,
 *   so equal inputs give equal bits, whatever the scheduling.
 * ws: effq_label_clean_ws_bytes(D, H, W) bytes: 4 B of label, 4 B of size and 1 B of mask per voxel, and 4.2 KB of
 *   counters - 80 MB for 155 x 240 x 240; 0 for dimensions out of range.  Limits: effq_cc_label's with P = 1.  Bad
 *   arguments (a null pointer, R out of range, an unknown op, N < 1, TO out of range or in its own set, sets[r][0] set, a
 *   connectivity other than 6 or 26, dimensions out of range) return EFFQ_ERR_ARG, a short workspace
 *   EFFQ_ERR_WORKSPACE; both launch nothing and leave out and stats as they were. */
#define EFFQ_LABEL_CLEAN_MAX_RULES 8
#define EFFQ_LABEL_CLEAN_LARGEST 0
#define EFFQ_LABEL_CLEAN_MIN 1
size_t effq_label_clean_ws_bytes(int D, int H, int W);
int effq_label_clean(const uint8_t* in, int D, int H, int W, int connectivity, int R, const uint8_t* sets,
                     const long long* rules, uint8_t* out, long long* stats, void* ws, size_t ws_bytes, void* stream);

/* ---- filling holes and closing or opening masks by a ball (--post fill, closeR, openR).  Arguments,
 * layout and meaning as effq_label_clean; ops EFFQ_LABEL_CLEAN_LARGEST and EFFQ_LABEL_CLEAN_MIN run the same launches
 * and give the same bits as there.  M = the voxels whose value is in the rule's set, on the map the previous rule left;
 * B_R = {(dd, dh, dw): dd^2 + dh^2 + dw^2 <= R^2}, R = N in voxels, 1 <= R <= EFFQ_LABEL_POST_MAX_RADIUS.
 *   EFFQ_LABEL_POST_FILL: every hole of M becomes TO (N ignored).  A hole is a connected component of the voxels not in
 *     M that holds no voxel on any of the six faces of the volume; the holes are connected by the dual of `connectivity`
 *     (6 when the rules use 26, 26 when they use 6).  Every voxel of a hole becomes TO whatever value it had.  An axis of
 *     extent 1 leaves no holes.
 *   EFFQ_LABEL_POST_CLOSE: the voxels of (M + B_R) - B_R (dilation, then erosion) that are not in M become TO.
 *   EFFQ_LABEL_POST_OPEN: the voxels of M that are not in (M - B_R) + B_R (erosion, then dilation) become TO.
 *     Both are taken on the infinite grid with everything outside the volume background, and restricted to the volume:
 *     closing is extensive and idempotent (a mask closer than R to a face does not grow towards it), opening is
 *     anti-extensive and idempotent.
 *   TO is 0..255; for FILL and CLOSE, which add to the mask, it is one of the rule's set, for the other ops it is not.
 * stats (R, 2) int64 on the device: FILL - the holes filled, the voxels relabelled; CLOSE and OPEN - the voxels of M
 *   before the rule, the voxels relabelled; LARGEST and MIN as effq_label_clean.
 * Per rule: FILL - the complement plane (one launch), the five labelling launches at the dual connectivity, the voxels
 *   of the faces marking their roots, and one pass that rewrites and counts: 8 launches.  CLOSE, OPEN - dilation and
 *   erosion are thresholds of the exact squared distance (effq_edt_sq's three launches): dilate(X) = {edt_sq(., X) <=
 *   R^2}, erode(X) = {edt_sq(., complement of X) > R^2}, both on the plane padded by R voxels on every side (background
 *   for CLOSE, sites of the complement for OPEN), which makes them those of the infinite grid: a memset and 9 launches
 *   (sites, transform, threshold, transform, rewrite and count).  One launch zeroes the counters first (and a device
 *   copy when out is not in).  All on `stream`, no read by the host and no workgroup that waits for another.  Integer
 *   compares, adds and a max only, so equal inputs give equal bits, whatever the scheduling.
 * ws: effq_label_post_ws_bytes(D, H, W, max_radius) bytes, max_radius = the largest R of the CLOSE and OPEN rules, 0
 *   without one: effq_label_clean_ws_bytes(D, H, W) and 16 B, and for max_radius > 0 1 B of site and 4 B of squared
 *   distance per voxel of the padded plane (D + 2 max_radius)(H + 2 max_radius)(W + 2 max_radius), each rounded up to
 *   16 B - 129 071 568 B for 155 x 240 x 240 at radius 3 (80 MB without a ball).  0 for max_radius outside 0..32 or
 *   dimensions out of range.  Limits: effq_cc_label's with P = 1, and effq_edt_sq's with P = 1 for the padded plane
 *   (fewer than 2^31 voxels).  Bad arguments (a null pointer, R out of range, an unknown op, N < 1 for MIN, a radius
 *   outside 1..32, TO out of range, in the set for LARGEST, MIN and OPEN or outside it for FILL and CLOSE, sets[r][0]
 *   set, a connectivity other than 6 or 26, dimensions out of range) return EFFQ_ERR_ARG, a short workspace
 *   EFFQ_ERR_WORKSPACE; both launch nothing and leave out and stats as they were. */
#define EFFQ_LABEL_POST_FILL 2
#define EFFQ_LABEL_POST_CLOSE 3
#define EFFQ_LABEL_POST_OPEN 4
#define EFFQ_LABEL_POST_MAX_RADIUS 32
size_t effq_label_post_ws_bytes(int D, int H, int W, int max_radius);
int effq_label_post(const uint8_t* in, int D, int H, int W, int connectivity, int R, const uint8_t* sets,
                    const long long* rules, uint8_t* out, long long* stats, void* ws, size_t ws_bytes, void* stream);

/* Tallies of a label map (the score of a cleaned map): pred (S) uint8 label values against the truth -> counts (C, 4)
 * int64 = TP, FP, FN, TN per class, the layout of effq_seg_tallies.  lut: 256 uint16 on the host, read before the call
 * returns; bit c set = that label value belongs to class c.  The class bits of a predicted voxel are lut[pred[v]]; those
 * of the truth are lut[truth[v]] when truth_planes == 0 (truth (S) label values), and otherwise bit c is
 * truth[c * S + v] != 0 (truth (C, S) 0/1 planes).  1 <= C <= EFFQ_SEG_TALLIES_MAX_CLASSES, S < 2^40.  Per-workgroup
 * integer partials, added in block order by a second launch: equal inputs give equal bits.  4-B loads when pred and
 * truth are 4-B aligned (and S % 4 == 0 for planes), the last S % 4 voxels one by one.  ws:
 * effq_label_tallies_ws_bytes() of scratch; a shorter one returns EFFQ_ERR_WORKSPACE. */
size_t effq_label_tallies_ws_bytes(void);
int effq_label_tallies(const uint8_t* pred, const uint8_t* truth, int truth_planes, int C, long long S,
                       const uint16_t* lut, long long* counts, void* ws, size_t ws_bytes, void* stream);

/* ---- exact Euclidean distance transform of 3-D masks and the surface-distance columns of the validation
 * (validate_seg(..., surface=True): hd, hd95, assd per class; the reference has no counterpart, the definitions are
 * DESIGN section 13's).  Voxel units.  Separable and in integers throughout, so the squared distances are exact: along
 * w the distance to the nearest site of the row (one wave per row, ballots), then along h and along d the lower envelope
 * min_j (g(j) + (i - j)^2) of every line, a slab of lines staged in LDS and searched outwards from each voxel until
 * (i - j)^2 reaches the best value so far.  Three launches for effq_edt_sq; effq_seg_surface adds the decision bits, the
 * surface stencil, the zeroing and the filling of the histograms and their walk: eight, all on `stream`, no read by the
 * host and no workgroup that waits for another.
 *
 * effq_edt_sq: masks (P, D, H, W) uint8, non-zero = site -> sq (P, D, H, W) int32: the squared Euclidean distance of
 *   every voxel to the nearest site of its own plane (0 on a site), INT32_MAX everywhere in a plane without sites.
 *   P * D*H*W < 2^31, P <= 65535, D^2 + H^2 + W^2 < 2^31 (every distance fits), D and H <= EFFQ_EDT_MAX_LINE (a line
 *   of the h and d passes is staged in the LDS of one workgroup).
 * effq_seg_surface: stitched logits (C, D, H, W) of one case and its label, arguments as effq_seg_tallies.  Per class
 *   P = the predicted mask, L = the label mask (the tallies' own decisions; in argmax mode class 0 is a class like any
 *   other), S(M) = the voxels of M with a face neighbour that is background or outside the volume, E_M(v) = the squared
 *   distance of v to the nearest voxel of S(M).  counts (C, 6) int64 = nP, nL (voxels of S(P), S(L)), maxsq_PL,
 *   maxsq_LP (the largest E_L over S(P), the largest E_P over S(L); 0 where the set or the target is empty), qlo_sq,
 *   qhi_sq (the squared distances at ranks lo and min(lo + 1, n - 1) of the n = nP + nL pooled values in ascending
 *   order, lo = 95 (n - 1) / 100 in integers; 0 when a surface is empty); sums (C, 2) fp64 = the sum of sqrt(E_L) over
 *   S(P) and of sqrt(E_P) over S(L) (0 where the target is empty), added per bin of a histogram over E in a fixed
 *   order: equal inputs give equal bits.  hd, hd95 and assd follow on the host (evaluate.surface_metrics).
 * ws: effq_surf_ws_bytes(P, D, H, W) bytes for either call, P = 2 C for effq_seg_surface: 4 B of squared distance per
 *   plane and voxel, 2 B of decision bits and 2 B of surface bits per voxel, and per plane a histogram of
 *   (D-1)^2 + (H-1)^2 + (W-1)^2 + 2 counters (effq_edt_sq writes into `sq` and only checks the size).  A BraTS case
 *   (3 classes, 155 x 240 x 240): 214 MB of distances, 253 MB in all.  Bad arguments and a short workspace return
 *   EFFQ_ERR_ARG and launch nothing. */
#define EFFQ_EDT_MAX_LINE 16382
size_t effq_surf_ws_bytes(int P, int D, int H, int W);
int effq_edt_sq(const uint8_t* masks, int P, int D, int H, int W, int32_t* sq, void* ws, size_t ws_bytes, void* stream);
int effq_seg_surface(const float* logits, const uint8_t* label, int C, int D, int H, int W, int mode, int fuse,
                     float thresh, long long* counts, double* sums, void* ws, size_t ws_bytes, void* stream);

/* ---- the distance transform with per-axis weights and the surface distances in millimetres (validate_seg(...,
 * surface=True, geometry=...): the voxels of a scan are rarely cubes).  The squared distance of voxel v to site s is
 * defined in fp32, term by term:
 *     E(v, s) = fl( fl( fl(ww dw^2) + fl(wh dh^2) ) + fl(wd dd^2) ),   (dd, dh, dw) = v - s,
 * every fl one correctly rounded fp32 operation, no fused multiply-add, fp32 denormals kept.  The separable transform
 * (w, then h, then d) returns the bits of the brute force over all sites (DESIGN section 13 has the argument).  The
 * contract holds for the build of csrc/Makefile only: a recipe without -ffp-contract=off, or one that flushes fp32
 * denormals (-fgpu-flush-denormals-to-zero), may fuse or flush and then returns other bits.
 * wd, wh, ww: the squared spacing of the axes, float32(float64(spacing) ** 2); finite and > 0.
 *
 * effq_edt_sq_mm: masks (P, D, H, W) uint8, non-zero = site -> sq (P, D, H, W) fp32 = min over the sites s of the
 *   voxel's own plane of E(v, s); +inf everywhere in a plane without sites.  P * D*H*W < 2^31, P <= 65535, every extent
 *   <= EFFQ_EDT_MM_MAX_EXTENT ((i - j)^2 < 2^24 is exact in fp32).  Three launches.
 * effq_seg_surface_mm: arguments, decisions, P, L and S(M) as effq_seg_surface.  counts (C, 2) int64 = nP, nL; sq (C, 4)
 *   fp32 = the largest E_L over S(P), the largest E_P over S(L) (0 where the set or the target is empty) and the values
 *   at ranks lo and min(lo + 1, n - 1) of the n = nP + nL pooled values in ascending order, lo = 95 (n - 1) / 100 in
 *   integers (0 where a surface is empty); sums (C, 2) fp64 = the sum of sqrt((double)E_L) over S(P) and of
 *   sqrt((double)E_P) over S(L) (0 where the target is empty).  Integer counts select the two ranks and the
 *   sums are added in a fixed order: equal inputs give equal bits.  A fixed number of launches on `stream`, no read by
 *   the host and no workgroup that waits for another.  hd, hd95 and assd follow on the host (evaluate.surface_metrics_mm).
 * ws: effq_surf_mm_ws_bytes(P, D, H, W) bytes for either call, P = 2 C for effq_seg_surface_mm: 4 B of squared distance
 *   per plane and voxel, 2 B of decision bits and 2 B of surface bits per voxel and 161 KiB of counters and partial sums
 *   (effq_edt_sq_mm writes into `sq` and only checks the size); 0 for dimensions out of range.  A BraTS case (3 classes,
 *   155 x 240 x 240): 214 MB of distances, 250 MB in all.  Bad arguments (a weight that is 0, negative, NaN or infinite
 *   among them) and a short workspace return EFFQ_ERR_ARG and launch nothing. */
#define EFFQ_EDT_MM_MAX_EXTENT 4096
size_t effq_surf_mm_ws_bytes(int P, int D, int H, int W);
int effq_edt_sq_mm(const uint8_t* masks, int P, int D, int H, int W, float wd, float wh, float ww, float* sq, void* ws,
                   size_t ws_bytes, void* stream);
int effq_seg_surface_mm(const float* logits, const uint8_t* label, int C, int D, int H, int W, int mode, int fuse,
                        float thresh, float wd, float wh, float ww, long long* counts, float* sq, double* sums, void* ws,
                        size_t ws_bytes, void* stream);

/* ---- scoring a finished label map against a label map on one grid (the `score` mission).  pred and
 * truth (D, H, W) uint8 label values; lut: 256 uint16 on the host, read before the call returns, bit c set = that label
 * value belongs to class c (effq_label_tallies' table; a voxel may sit in several classes), every entry < 1 << C.  One
 * launch makes the decision bits of seg_masks.h from the two maps, bits[v] = (lut[pred[v]] & 0xff) | (lut[truth[v]] & 0xff)
 * << 8 (4-B loads and one 8-B store when both maps are 4-B aligned, the last S % 4 voxels one by one); everything after
 * it is the launches of the entry point that takes logits, on those bits.  1 <= C <= EFFQ_SEG_TALLIES_MAX_CLASSES.  The
 * Dice tallies of the same maps are effq_label_tallies'.
 *
 * effq_label_lesions: counts (C, 4) int64 = totall, predl, fnl, fpl, meaning and layout of effq_seg_lesions.  ws:
 *   effq_cc_ws_bytes(2 C, D, H, W).  Bad arguments (those of effq_seg_lesions, a table entry with a bit at or above C)
 *   return EFFQ_ERR_ARG, a short workspace EFFQ_ERR_WORKSPACE; both launch nothing and leave counts as it was.
 * effq_label_surface_mm: P, L, S(M), E_M, the weights and counts (C, 2), sq (C, 4), sums (C, 2) as effq_seg_surface_mm:
 *   for equal decision bits the same launches and the same bits.  tol_sq: ntol fp32 squared tolerances in mm^2 on the
 *   host, read before the call returns, float32(float64(tol_mm) ** 2); 0 <= ntol <= EFFQ_SURF_TOL_MAX, each finite and
 *   >= 0, strictly ascending.  within (C, 2, ntol) int64: within[c][0][k] = the voxels of S(P) of class c with E_L(v) <=
 *   tol_sq[k], within[c][1][k] = those of S(L) with E_P(v) <= tol_sq[k]; the comparison is in fp32 on the stored
 *   distance, and a +inf distance (the target has no surface) is never within.  The normalised surface Dice at
 *   tolerance k is (within[c][0][k] + within[c][1][k]) / (nP + nL) on the host.  ntol == 0 launches nothing for it and
 *   leaves within untouched; it may then be null.  Two more launches: every surface voxel adds 1 at the first tolerance
 *   that holds it in LDS counters of its workgroup, which are added to int64 counters of the workspace; one small launch
 *   takes the prefix sums.  Integer adds only: equal inputs give equal bits.  No read by the host, no workgroup that
 *   waits for another.
 *   ws: effq_label_surface_mm_ws_bytes(C, D, H, W, ntol) bytes, 16-B aligned: effq_surf_mm_ws_bytes(2 C, D, H, W) and
 *   1152 B of counters; 0 for what the call refuses.  It may hold anything on entry.  Bad arguments (those of
 *   effq_seg_surface_mm, a table entry with a bit at or above C, ntol out of range, a tolerance that is negative, NaN,
 *   infinite or not above the one before it) and a short workspace return EFFQ_ERR_ARG, launch nothing and leave every
 *   output as it was. */
#define EFFQ_SURF_TOL_MAX 8
int effq_label_lesions(const uint8_t* pred, const uint8_t* truth, int C, int D, int H, int W, const uint16_t* lut,
                       int connectivity, long long* counts, void* ws, size_t ws_bytes, void* stream);
size_t effq_label_surface_mm_ws_bytes(int C, int D, int H, int W, int ntol);
int effq_label_surface_mm(const uint8_t* pred, const uint8_t* truth, int C, int D, int H, int W, const uint16_t* lut,
                          float wd, float wh, float ww, const float* tol_sq, int ntol, long long* counts, float* sq,
                          double* sums, long long* within, void* ws, size_t ws_bytes, void* stream);

/* ---- one geometric record per lesion of finished label maps (`score --lesion_measures`, `predict --lesion_measures`;
 * DESIGN section 28).  pred, truth, lut, C and connectivity as effq_label_lesions.  With truth there are P = 2 C planes,
 * plane q < C the predicted mask of class q and plane C + q its label mask, and counts (C, 4) is bit for bit
 * effq_label_lesions'.  With truth null only the P = C predicted planes exist, counts may be null and every overlap is 0.
 * wd, wh, ww: the fp32 axis weights float32(float64(spacing) ** 2), finite and > 0.  slice_axis 0, 1 or 2: the array
 * axis the slices are stacked along.  Every extent <= EFFQ_EDT_MM_MAX_EXTENT, P D H W < 2^31, P max_rows < 2^31.
 *
 * nrows (P) int64 and rows (P, max_rows, 3) int32 = first voxel, size, overlap: the contract of effq_seg_lesion_table
 *   (row k is the component whose first voxel has the k-th smallest linear index, nrows is the true count, of a plane
 *   with more rows than fit the first max_rows are complete, rows past nrows are untouched).
 * meas (P, max_rows, EFFQ_LESION_MEASURE_WORDS) int64, one record per row that fits, nothing else written:
 *   0..2   the sums of d, h and w over the voxels of the component (integer adds)
 *   3..8   its box: the least d, h, w, then the greatest d, h, w (inclusive)
 *   9, 10  the linear indices a <= b of two voxels of the component that attain the greatest
 *          E = (wd * f(dd^2) + wh * f(dh^2)) + ww * f(dw^2) over all its pairs of voxels: (dd, dh, dw) the integer
 *          offsets, f the exact conversion of the square to fp32, every product and sum rounded to fp32
 *   11, 12 the same over the pairs that share the coordinate along slice_axis
 *   A component of one voxel has a = b = that voxel (distances run between voxel centres).  The diameters in mm follow
 *   on the host from the end points and the spacing.
 * Only the voxels that end a line of the component along w (along h when slice_axis is 2) enter the search: E is
 *   strictly convex along a line and rounding is monotone, so the fp32 maximum over them is the one over all voxels.
 *   Among the pairs of line ends of the greatest E, a is the least index any of them holds and b the least partner of
 *   a at that E (an inner voxel of a line may reach the same fp32 E after rounding; it is never returned).
 *   Integer atomics only, their winners decided by value: equal inputs give equal bits, whatever the workspace holds
 *   on entry.  A fixed number of launches on `stream`, no read by the host, no workgroup that waits for another.
 * The search walks the line ends of a component in tiles of 256 and costs 65536 pairs per pair of tiles (i <= j): it
 *   grows with the square of the line ends of one component.  A call whose rows that fit have more than
 *   EFFQ_LESION_MEASURE_MAX_TILE_PAIRS tile pairs in all (4.4e12 voxel pairs; one solid component of 512^3 has 2.1e6, a
 *   map of noise that hangs together has more) does not run it: slots 9..12 of every record are then -1 and the rest
 *   of the call's outputs is complete.  The bound is on the work of one launch, not on the volume.
 * ws: effq_label_lesion_measures_ws_bytes(C, planes, D, H, W, max_rows) bytes, planes = P, 16-B aligned:
 *   effq_cc_table_ws_bytes(P, D, H, W, max_rows), 4 B per plane and voxel for the compacted line ends and 36 B per
 *   plane and row; 0 for what the call refuses.  Bad arguments (those of effq_label_lesions, a slice_axis other than 0,
 *   1, 2, a weight that is 0, negative, NaN or infinite, an extent above the limit, max_rows <= 0, a null meas, rows or
 *   nrows, a null counts with a truth map) return EFFQ_ERR_ARG, a short workspace EFFQ_ERR_WORKSPACE; both launch
 *   nothing and leave every output as it was. */
#define EFFQ_LESION_MEASURE_WORDS 13
#define EFFQ_LESION_MEASURE_MAX_TILE_PAIRS (1ll << 26)
size_t effq_label_lesion_measures_ws_bytes(int C, int planes, int D, int H, int W, int max_rows);
int effq_label_lesion_measures(const uint8_t* pred, const uint8_t* truth, int C, int D, int H, int W,
                               const uint16_t* lut, int connectivity, float wd, float wh, float ww, int slice_axis,
                               int max_rows, long long* counts, long long* nrows, int32_t* rows, long long* meas,
                               void* ws, size_t ws_bytes, void* stream);

/* ---- the `prep` mission (prep.py): source scans to the standardised, cropped arrays the `ptq` mission reads.  One
 * subject at a time: x (C, D, H, W) fp32, contiguous, S = D H W voxels per modality, C <= EFFQ_PREP_MAX_MODALITIES,
 * C S < 2^31, every extent <= 32767.  mask_mode EFFQ_PREP_MASK_NONZERO: the mask of modality c is x_c != 0 (a NaN is
 * inside); EFFQ_PREP_MASK_ALL: every voxel.  All pointers are device memory except pmin / pmax (three host ints each,
 * read before the call returns).  Reductions go through per-workgroup partials in `ws` (EFFQ_PREP_WS_BYTES, 8-B aligned)
 * and one finishing workgroup that adds them in block order: no floating-point atomics, equal inputs give equal bits.
 * fp32 pointers need 4-B alignment only (16-B accesses go through a type of that alignment).  Nothing is read by the
 * host, no workgroup waits for another; bad arguments return EFFQ_ERR_ARG and launch nothing.
 *
 * window:  x[i] = x[i] < lo ? lo : x[i] > hi ? hi : x[i] in place (numpy.clip; a NaN stays), lo <= hi.
 * resample: x (N, D, H, W) -> y (N, OD, OH, OW) with the factors f = target spacing / source spacing per axis; the
 *   caller gives the output extents (prep.resample_extent).  Output index o of an axis of source extent n:
 *   EFFQ_PREP_LINEAR (fp32 in and out): s = (o + 0.5) f - 0.5 in fp64, clamped to [0, n - 1]; i0 = floor(s), i1 =
 *     min(i0 + 1, n - 1), l1 = float(s - i0), l0 = 1.0f - l1; the eight neighbours are combined in fp32 as
 *     l0d (l0h (l0w v000 + l1w v001) + l1h (l0w v010 + l1w v011)) + l1d (...), nothing fused.  No filter before
 *     down-sampling: that is effq_prep_smooth below, a call of its own.
 *   EFFQ_PREP_NEAREST (uint8 in and out): index min(n - 1, floor((o + 0.5) f)) per axis.
 * bbox_moments (pass 1): bbox_out[6] int32 = the least d, h, w and the greatest d, h, w of the union of the modalities'
 *   masks (the whole grid for MASK_ALL; least = the extent and greatest = -1 when the union is empty); count_out[C]
 *   int64 and sum_out[C] fp64 = the voxels of modality c's own mask and the sum of their values.  Two launches.
 * sqdev (pass 2): sqdev_out[C] fp64 = sum over the mask of (double(x) - mean[c])^2.  Two launches.
 * standardise_crop (pass 3): y (C, pmax - pmin) = mask ? float((double(x) - mean[c]) / std[c]) : +0.0f over the box
 *   pmin <= (d, h, w) < pmax.
 * crop_u8: the same box of C uint8 volumes (the label).
 * union_mask: mask (S) uint8 = 1 where any modality's mask holds, else 0. */
#define EFFQ_PREP_MAX_MODALITIES 4
#define EFFQ_PREP_WS_BYTES (1024 * (2 * EFFQ_PREP_MAX_MODALITIES * 8 + 8 * 4))
enum { EFFQ_PREP_MASK_NONZERO = 0, EFFQ_PREP_MASK_ALL = 1 };
enum { EFFQ_PREP_LINEAR = 0, EFFQ_PREP_NEAREST = 1 };
int effq_prep_window(float* x, size_t n, float lo, float hi, void* stream);
int effq_prep_resample(const void* x, int N, int D, int H, int W, double fd, double fh, double fw, int mode, void* y,
                       int OD, int OH, int OW, void* stream);
int effq_prep_bbox_moments(const float* x, int C, int D, int H, int W, int mask_mode, int* bbox_out, long long* count_out,
                           double* sum_out, void* ws, size_t ws_bytes, void* stream);
int effq_prep_sqdev(const float* x, int C, long long S, int mask_mode, const double* mean, double* sqdev_out, void* ws,
                    size_t ws_bytes, void* stream);
int effq_prep_standardise_crop(const float* x, int C, int D, int H, int W, int mask_mode, const int* pmin,
                               const int* pmax, const double* mean, const double* stdev, float* y, void* stream);
int effq_prep_crop_u8(const uint8_t* x, int C, int D, int H, int W, const int* pmin, const int* pmax, uint8_t* y,
                      void* stream);
int effq_prep_union_mask(const float* x, int C, long long S, int mask_mode, uint8_t* mask, void* stream);

/* ---- the percentile window (csrc/prep_quantile.hip; prep.py --prep_window pLO,pHI, where the rule is defined): every
 * modality is clipped to a pair of its own percentiles over its own mask.  The rule, restated: the n voxels of modality
 * c's mask (mask_mode as above) are sorted ascending, -Inf first, -0.0 counted as +0.0, every NaN after +Inf.  For a
 * percentile q in [0, 100], all in fp64 with the product first: h = (n - 1) q / 100, k = floor(h), a = sorted[k],
 * b = sorted[min(k + 1, n - 1)], v = a when a == b, else a + (h - k) (b - a); the bound is the fp32 value nearest v
 * (numpy's default `linear` method, up to the rounding of h).  The voxels inside the mask are then clipped to [lo, hi],
 * those outside it are left alone; the host stops at n < 2, at a bound that is not finite and, with MASK_NONZERO, at a
 * bound of exactly 0 (it would move voxels out of the mask).
 *
 * effq_prep_quantiles: the device half.  x (C, S) fp32 under the limits above (C <= EFFQ_PREP_MAX_MODALITIES, C S < 2^31,
 *   4-B aligned); q: R HOST doubles in [0, 100], 1 <= R <= EFFQ_PREP_QUANTILE_MAX, read before the call returns.
 *   count_out[c] int64 = n; stat_out[c][r][0..1] fp32 = a and b for q[r], with k formed on the device in fp64 from the
 *   count it found; both are NaN when n = 0, a zero of either sign is returned as +0.0, a NaN as a quiet NaN.  The host
 *   interpolates (prep.percentile_value).  Method: a radix select over the order-preserving 32-bit key of the float, most
 *   significant digit first, 8 bits in four passes.  Each pass streams x and counts the next digit of the voxels under
 *   the prefixes still followed (up to 2 R, targets with equal prefixes share one) in 32-bit LDS counters per workgroup,
 *   equal digits of a wave combined by ballot first; the workgroups' totals are combined in `ws` by integer atomics, and
 *   a one-workgroup step picks each target's digit and remaining rank.  Nine launches on `stream`; nothing is read by
 *   the host, no workgroup waits for another, no floating-point atomic: equal inputs give equal bits.  `ws`:
 *   *bytes of effq_prep_quantile_ws_bytes (as effq_prep_cubic_ws_bytes reports its own), 8-B aligned, any contents (the
 *   call clears what it counts in).
 * effq_prep_mask_window: x[i] = in_mask(x[i]) ? clip(x[i]) : x[i] in place over n floats, clip that of effq_prep_window
 *   (a NaN stays), lo <= hi.
 * Refused with EFFQ_ERR_ARG before any launch: a null pointer, C or S out of range, a mask_mode that is neither, R outside
 * 1 ... EFFQ_PREP_QUANTILE_MAX, a q outside [0, 100] or NaN, a workspace that is too short or not aligned to 8 B, x or
 * stat_out not aligned to 4 B, count_out not aligned to 8 B, lo > hi or a NaN bound. */
#define EFFQ_PREP_QUANTILE_MAX 4
int effq_prep_quantile_ws_bytes(size_t* bytes);
int effq_prep_quantiles(const float* x, int C, long long S, int mask_mode, const double* q, int R, long long* count_out,
                        float* stat_out, void* ws, size_t ws_bytes, void* stream);
int effq_prep_mask_window(float* x, size_t n, float lo, float hi, int mask_mode, void* stream);

/* ---- the anti-alias filter before down-sampling (csrc/prep_smooth.hip; prep.py --prep_antialias): a separable Gaussian
 * on the source grid, x (N, D, H, W) fp32 -> y of the same shape.  Per array axis a with the factor f_a = target spacing /
 * source spacing of the resampling that follows (the caller's rule, prep.antialias_taps):
 *   sigma_a = (f_a - 1) / 2 if f_a > 1, else 0 (an axis that is kept or up-sampled is not filtered);
 *   r_a = int(4 sigma_a + 0.5) (scipy's truncate = 4.0); an axis with r_a = 0 is not filtered, whatever sigma_a is;
 *   g_k = exp(-k^2 / (2 sigma_a^2)), k = -r_a .. r_a, in fp64 on the host, normalised to sum 1, then rounded to fp32
 *     and not normalised again: the fp32 taps sum to 1 within (2 r_a + 1) 2^-24.
 * taps_d, taps_h, taps_w are HOST arrays of r + 1 floats, g_0 first (g_-k = g_k), each in (0, 1]; they are read before
 * the call returns and travel in the launch parameters: no device allocation, no copy.  taps of an axis with r = 0 are
 * not read and may be null.  Along a filtered axis of extent n
 *   y[i] = sum_k g_k x[clamp(i + k, 0, n - 1)]
 * (edge replication, scipy's mode = 'nearest', the clamping of EFFQ_PREP_LINEAR; n < r is legal), formed in fp32 as
 * acc = g_0 x[i], then acc = fmaf(g_k, x[clamp(i - k)] + x[clamp(i + k)], acc) for k = 1 .. r.  The filtered axes are
 * applied one after the other, W then H then D, one launch each, fp32 stored between them: the first of three passes
 * writes y, the one before the last writes tmp, the last writes y.  tmp (N D H W floats) may be null when at most one
 * axis is filtered; no other device memory is used.  keep_zero = 1: a voxel whose value in x is exactly 0.0f (either
 * sign) is exactly +0.0f in y, whatever its neighbours hold, so a zero background does not take up the body's values
 * (x is read again in the last pass for this).  A NaN or an Inf spreads to every voxel within the radius along each
 * filtered axis; nothing treats them specially.  The grid depends on the extents alone and there is no atomic: equal
 * inputs give equal bits.  Refused with EFFQ_ERR_ARG before any launch: a null x or y, extents outside those of the
 * prep kernels (N D H W < 2^31, every extent <= 32767), a radius outside 0 ... EFFQ_PREP_SMOOTH_MAX_RADIUS, all three
 * radii 0 (nothing to do), null or non-finite taps of a filtered axis, keep_zero other than 0 and 1, a null tmp when two
 * or three axes are filtered, a pointer not aligned to 4 B, and x, y, tmp overlapping one another. */
#define EFFQ_PREP_SMOOTH_MAX_RADIUS 32
int effq_prep_smooth(const float* x, int N, int D, int H, int W, const float* taps_d, int rd, const float* taps_h, int rh,
                     const float* taps_w, int rw, int keep_zero, float* y, float* tmp, void* stream);

/* ---- cubic B-spline resampling (csrc/prep_spline.hip; prep.py --prep_interp cubic, where the rule is defined):
 * x (N, D, H, W) fp32 -> y (N, OD, OH, OW) fp32 with the factors and the output extents of effq_prep_resample; x is not
 * modified.  The extents of x and of y obey the limits of the prep kernels (N D H W < 2^31, every extent <= 32767).
 * 1 Prefilter, the B-spline coefficient transform, along D, then H, then W, in fp64 into `ws`
 *   (*bytes of effq_prep_cubic_ws_bytes = 8 N D H W, 8-B aligned).  Per axis of extent n >= 2 the coefficients solve
 *   (c[k-1] + 4 c[k] + c[k+1]) / 6 = x[k] with the whole-sample mirror c[-1] = c[1], c[n] = c[n-2] (scipy's
 *   mode='mirror'), by the recursion with the pole z = sqrt(3) - 2 and the gain 6:
 *     c+[0] = 6 s / (1 - z^(2n-2)),  s = sum_{k=0}^{2n-3} z^k xm[k],  xm the mirrored line (xm[k] = x[k] for k < n,
 *       x[2n-2-k] after it): the exact sum over the period, no truncated horizon (a term whose power z^k, formed by
 *       repeated multiplication, has underflowed to 0 in fp64 is 0 and is not visited);
 *     c+[k] = 6 x[k] + z c+[k-1];   c[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]);   c[k] = z (c[k+1] - c+[k]).
 *   An axis of extent 1 is not filtered; all three axes are filtered whatever their factors.
 * 2 Evaluation.  Output index o of an axis sits at s = (o + 0.5) f - 0.5 in fp64, clamped to [0, n - 1] (the coordinate
 *   of EFFQ_PREP_LINEAR); i0 = floor(s), t = s - i0; the weights on c[i0-1 .. i0+2] are (1-t)^3 / 6,
 *   (3t^3 - 6t^2 + 4) / 6, (-3t^3 + 3t^2 + 3t + 1) / 6, t^3 / 6, the indices -1 and n mirrored (an index still outside
 *   after that has weight 0 and is clamped); on an axis of extent 1 the one coefficient has weight 1.  The 64
 *   coefficients are combined in fp64 in one fixed order, w innermost, then h, then d: the four products of a row are
 *   added in index order, the four row sums times their h weights likewise, then the four plane sums times their d
 *   weights; the sum is rounded to fp32 once.  Nothing is fused.
 * 3 zero_keep = 1: an output voxel is exactly +0.0f when every source voxel of its trilinear footprint is exactly 0
 *   (per axis i0 and i0 + 1, the second only when s > i0 and i0 < n - 1; a NaN is not 0), so a zero background stays
 *   exactly zero and the body reaches no further than under EFFQ_PREP_LINEAR.  zero_keep = 0: no voxel is treated so.
 * A NaN or an Inf is carried along its whole lines by the recursions, and from there over the volume.
 * Four launches (three prefilter passes, one evaluation), no atomics, grids that depend on the extents alone: equal
 * inputs give equal bits.  Refused with EFFQ_ERR_ARG before any launch: a null x, y or ws, extents outside the limits, x
 * or y not aligned to 4 B, ws not aligned to 8 B, ws_bytes below what effq_prep_cubic_ws_bytes gives (itself refused
 * for extents outside the limits), a factor outside (0, 1e6] or NaN, zero_keep other than 0 and 1.
 * effq_prep_cubic_plan (launches nothing): *chunk = the voxels of a row the W pass visits at a time, *tile_rows = the rows
 * of one of its tiles; items[4] = the work items of the D, H and W prefilter passes (lines, lines, rows; 0 for a pass that
 * is not launched: H = 1, W = 1) and of the evaluation (groups of four output voxels along W); trip[4] = how many of
 * them one trip of each launch's capped grid covers (items > trip: the grid-stride loop takes a further trip).
 * effq_prep_spline_prefilter: the passes of step 1 alone (`passes` = a sum of EFFQ_PREP_SPLINE_PASS_*; D reads x and writes
 * ws, H and W work in place in ws; x may be null without the D pass), for tests and profiles. */
enum { EFFQ_PREP_SPLINE_PASS_D = 1, EFFQ_PREP_SPLINE_PASS_H = 2, EFFQ_PREP_SPLINE_PASS_W = 4 };
int effq_prep_cubic_ws_bytes(int N, int D, int H, int W, size_t* bytes);
int effq_prep_cubic_plan(int N, int D, int H, int W, int OD, int OH, int OW, int* chunk, int* tile_rows, long long* items,
                         long long* trip);
int effq_prep_spline_prefilter(const float* x, int N, int D, int H, int W, int passes, void* ws, size_t ws_bytes,
                               void* stream);
int effq_prep_resample_cubic(const float* x, int N, int D, int H, int W, double fd, double fh, double fw, int zero_keep,
                             float* y, int OD, int OH, int OW, void* ws, size_t ws_bytes, void* stream);

/* ---- reorientation (csrc/reorient.hip; prep.py --prep_orient): x (N, D, H, W) -> y (N, dims[src_axis[0]],
 * dims[src_axis[1]], dims[src_axis[2]]) with dims = {D, H, W}: output axis p is source axis src_axis[p] (three host ints,
 * a permutation of 0, 1, 2, read before the call returns), reversed iff bit p of flip_mask is set:
 *   y[n][o0][o1][o2] = x[n][s],  s[src_axis[p]] = flip_mask >> p & 1 ? dims[src_axis[p]] - 1 - o_p : o_p.
 * elem_bytes 4 (fp32, moved as 32-bit words: a NaN keeps its payload) or 1 (uint8).  Two variants, which
 * effq_prep_reorient_plan reports in *variant without touching the device: 0 when src_axis[2] == 2 (source W stays the
 * innermost axis: rows are copied, 16 B per thread, reversed inside the vector, scalar tail), 1 otherwise (a tiled
 * transpose through LDS, flips applied to the destination coordinates of the tile).  One launch, no atomics, no
 * reductions: equal inputs give equal bits.  Refused with EFFQ_ERR_ARG before any launch: a null pointer, extents outside
 * 1 ... 32767, N D H W >= 2^31, elem_bytes other than 1 and 4, a src_axis that is no permutation, flip_mask outside
 * 0 ... 7, a pointer not aligned to elem_bytes, x and y overlapping.  uint8 volumes may start at any byte (a slice of a
 * larger buffer): their wider accesses go through types of 1-B alignment. */
int effq_prep_reorient(const void* x, int N, int D, int H, int W, const int* src_axis, int flip_mask, int elem_bytes,
                       void* y, void* stream);
int effq_prep_reorient_plan(const int* src_axis, int flip_mask, int elem_bytes, int* variant);

/* ---- alignment (csrc/prep_align.hip; prep.py --prep_align, where the rule is defined): one volume x (D, H, W) resampled
 * onto another grid y (OD, OH, OW) through a general affine.  m: 12 HOST doubles, a row-major 3 x 4 matrix that maps an
 * output voxel index (d, h, w, 1) to source voxel coordinates, read before the call returns.  Per output voxel and axis a,
 * in fp64 and in exactly this order, nothing fused:  s_a = ((m[a][0] d + m[a][1] h) + m[a][2] w) + m[a][3].
 * Field of view: the voxel is inside when -0.5 <= s_a < n_a - 0.5 on all three axes (n the source extent; `<` at the upper
 * end so that nearest never indexes n_a and the half voxel around every source voxel belongs to it alone); outside it
 * the output is +0.0f, or 0 for a label, and nothing is read.
 *   EFFQ_PREP_LINEAR (fp32 in and out), inside: c = clamp(s_a, 0, n_a - 1) (the edge replicated over the outer half
 *     voxel), i0 = floor(c), i1 = i0 + (i0 < n_a - 1), l1 = float(c - floor(c)), l0 = 1.0f - l1; the eight neighbours are
 *     combined in fp32 in the order of effq_prep_resample: l0d (l0h (l0w v000 + l1w v001) + l1h (...)) + l1d (...).  A
 *     NaN or an Inf among the eight reaches the output even at weight 0.
 *   EFFQ_PREP_NEAREST (uint8 in and out), inside: the index floor(s_a + 0.5), kept at n_a - 1 at most (the fp64 sum can
 *     round up to n_a only when n_a = 1).
 * inside (device, one int64, 8-B aligned): the number of output voxels inside the field of view.  The call zeroes it with
 * a memset on the stream; every workgroup sums its count in LDS and adds it once with an integer atomic: equal inputs give
 * equal bits, there is no floating-point atomic and no workgroup waits for another.  One launch; a thread makes four
 * consecutive w of an output row.  Refused with EFFQ_ERR_ARG before the memset and before any launch: a null pointer,
 * extents outside 1 ... 32767 or D H W >= 2^31 or OD OH OW >= 2^31, another mode, a matrix entry that is not finite, for
 * EFFQ_PREP_LINEAR an x or y that is not 4-B aligned, an `inside` that is not 8-B aligned. */
int effq_prep_align(const void* x, int D, int H, int W, const double* m, int mode, void* y, int OD, int OH, int OW,
                    long long* inside, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFQ_HIP_H */
